/* mi355x_qr.h -- public C ABI of libmi355xqr.so: MI355X-native (gfx950) fp64 blocked Householder QR.
 *
 * The library is a drop-in for the host entry points of brian-kelley/CUDA-QR's qr.c built with
 * Scalar = double ("double* A, m, n -> Q, R"), plus a device-resident API for callers that keep the
 * matrix in HBM (bench, TSQR over several GPUs).  Plain pointers and sizes only; no HIP, C++ or torch
 * types cross this boundary.  All matrices are column-major with leading dimension = row count unless
 * an ld argument says otherwise (reference layout, qr.c:35,85).
 *
 * Every entry point cites the reference interface it replaces as file:line into the reference repo.
 */
#ifndef MI355X_QR_H
#define MI355X_QR_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * 1. Drop-in symbols (same names, argument order and meaning as the reference, Scalar = double)
 * ------------------------------------------------------------------------------------------- */

/* replaces qr.c:47-53 getPanelDims.  The reference's sliding PR x PC window does not exist here: a
 * column panel of width nb (the library block size, default 128) is factored over its full height,
 * so rowPanels = 1 and colPanels = ceil(n/nb).  tau therefore holds rowPanels*colPanels*nb >= n
 * entries, which keeps the reference caller's tau[i*rowPanels + j] indexing (qr.c:483-490) in bounds. */
void getPanelDims(int m, int n, int* rowPanels, int* colPanels);

/* replaces qr.c:55-313 mmqr (and its GPU twin qr.cu:475-553).  In-place Householder QR of the m x n
 * (m >= n) host matrix `mat`: on return the upper triangle holds R and the sub-diagonal of column j
 * holds the tail of reflector v_j (v_j(j) = 1 implicit).  *tau is malloc'ed here (caller frees, as
 * qr.c:61,521) with colPanels*nb entries: tau[j] = Householder scalar of column j, zero padded.
 * tau is an opaque array consumed by this library's own explicitQR: the reference's
 * window-indexed layout (qr.c:300-304) depends on its compile-time PR, PC and is not reproduced.
 * Convention: LAPACK dlarfg (H = I - tau v v^T, R diagonal = -sign(x0)*||x||, same as qr.c:144-158),
 * except that an exactly-zero column tail gives tau = 0 where the reference yields NaN (qr.c:152). */
void mmqr(double* mat, double** tau, int m, int n);

/* replaces qr.c:330-438 explicitQR.  From mmqr's output builds R (m x n: upper triangle of A, zero
 * below, qr.c:334-343) and the dense m x m orthogonal Q = H_0 H_1 ... H_{n-1} (the reference forms it
 * with an m^3 product per reflector, qr.c:415-429; here: blocked backward accumulation on MFMA tiles).
 * Q and R are caller-allocated (qr.c:492-493). */
void explicitQR(double* A, double* tau, double* Q, double* R, int m, int n);

/* replaces qr.c:443-459 dgemm: C (k x n) = A (k x m) * B (m x n), column-major. Runs on the GPU. */
void dgemm(double* A, double* B, double* C, int k, int m, int n);

/* replaces qr.c:316-324 identity: A = I(m). */
void identity(double* A, int m);

/* replaces qr.c:21-33 printMat (row-by-row debug print to stdout, "%9f "). */
void printMat(double* mat, int m, int n);

/* The reference returns nothing and exits/asserts on error (qr.c:465, qr.cu:467-471).  The void
 * shims above print a diagnostic to stderr and return; these variants return a status instead
 * (0 = ok, >0 = hipError_t, <0 = QR_E_*).  The library never calls exit(). */
int mmqr_status(double* mat, double** tau, int m, int n);
int explicitQR_status(double* A, double* tau, double* Q, double* R, int m, int n);
int dgemm_status(double* A, double* B, double* C, int k, int m, int n);

/* Float instantiation (the reference as committed has Scalar = float, qr.c:11): mmqr / explicitQR on float
 * arrays with the same layouts and ownership rules.  The arithmetic is fp64 on the device (inputs widened, outputs rounded
 * once), so the results are at least as accurate as a float build of the reference.  The reference's window-indexed tau
 * layout (qr.c:300-304) is not what these return (it describes the reflectors of its sliding-window algorithm and cannot be
 * derived from a different reflector set): mmqr_legacy_status below runs that algorithm for callers who need it. */
void mmqr_f32(float* mat, float** tau, int m, int n);
void explicitQR_f32(float* A, float* tau, float* Q, float* R, int m, int n);
int mmqr_f32_status(float* mat, float** tau, int m, int n);
int explicitQR_f32_status(float* A, float* tau, float* Q, float* R, int m, int n);

/* Legacy-layout shim: the reference's sliding-window MMQR ITSELF on the device, with its compile-time window
 * PR x PC (qr.c:12-13) as arguments, for callers that consume the raw factored form -- the reflector tails exactly where qr.c:242-248
 * leaves them and tau[(rowPanels * pcCount + prCount) * PC + i] (qr.c:300-304; read by the reference's main, qr.c:483-490).
 * mmqr_legacy_status = qr.c:55-313, explicitQR_legacy_status = qr.c:330-438, getPanelDims_legacy = qr.c:47-53 for a given window.
 * Results equal the reference's to rounding (sums in wave-reduction order; tests: 1e-12 of the matrix scale), NaN for a zero column
 * like the reference (qr.c:152).  Shapes: what the reference's loops assume -- n % PC == 0, (m - PR) % (PR - PC) == 0, m >= PR --
 * with PR <= 64 and PC in {2, 4, 8, 16}; anything else is QR_E_ARG.  Two launches per column panel: a compatibility path, not a fast one. */
void getPanelDims_legacy(int m, int n, int PR, int PC, int* rowPanels, int* colPanels);
int mmqr_legacy_status(double* mat, double** tau, int m, int n, int PR, int PC);
int explicitQR_legacy_status(double* A, double* tau, double* Q, double* R, int m, int n, int PR, int PC);

#define QR_E_ARG      (-101)  /* bad argument (null pointer, m < n, non-positive size) */
#define QR_E_ALLOC    (-102)  /* host allocation failed */
#define QR_E_NODEVICE (-103)  /* no HIP device visible: there is NO CPU fallback */
#define QR_E_INTERNAL (-104)
#define QR_E_STALL    (-105)  /* qr_plan_sync: a hand-off between the workgroups of a one-launch panel timed out; the factorisation is invalid */
#define QR_E_REFUSED  (-106)  /* qr_plan_sync in latch mode (qr_plan_set_guard_mode): a full-width tall panel was refused; result invalid */
#define QR_E_SINGULAR (-107)  /* qr_lstsq: R(i,i) == 0 exactly for some i (LAPACK dgels INFO > 0); no solution was computed */
#define QR_E_NOCONV   (-108)  /* section 7: the Jacobi iteration did not reach its threshold in QR_JSVD_MAX_SWEEPS sweeps; results are not to be used */
#define QR_E_NOTPD    (-109)  /* section 6b: the row removal leaves no positive-definite triangle (rows that were never added, or too few left) */
const char* qr_strerror(int status);

/* Block sizes used by the drop-in entry points (outer compact-WY block nb: multiple of ib, <= 512, above 256 a multiple of 256;
 * leaf width ib <= 32).  Defaults 128 / 32; when nothing was set explicitly the outer block follows the shape: 256 where the two-stream
 * look-ahead schedule is used (n >= 2048, m n >= 8 M, not too tall) and from 8192 columns on, 64 for small square-ish problems
 * (n >= 512, m <= 3 n), 256 for taller ones of at most 8192 rows -- qr_default_block_size / getPanelDims(m, n, ..) report what that shape will really get;
 * env MI355XQR_NB / MI355XQR_IB override the defaults.
 * Threading: the library may be used from one host thread per GPU (each thread with its own current device and its own
 * plans; a plan belongs to one thread at a time).  Process-wide state (these defaults, per-device kernel attributes, the
 * plan cache of the host-pointer entry points) is guarded internally. */
int qr_set_block_size(int nb, int ib);
void qr_get_block_size(int* nb, int* ib);
/* the block sizes an m x n problem REALLY gets from mmqr / a plan created with nb = 0, ib = 0 (shape-dependent, see above):
 * mmqr's tau holds ceil(n / nb) * nb entries of this nb -- size buffers from here, not from qr_get_block_size */
int qr_default_block_size(int m, int n, int* nb, int* ib);

/* Thin QR for shapes whose m x m Q cannot exist (no reference counterpart: the
 * reference's explicitQR is m x m only).  A (m x n, host) is not modified; Q is m x n, R is n x n
 * (upper triangular, diag of any sign).  nshards > 1 factors `nshards` contiguous row blocks
 * independently and combines their R factors (TSQR on one device; the multi-GPU form of the same
 * steps is driven through the device API below with an RCCL all-gather between steps 1 and 2). */
int qr_thin(const double* A, int m, int n, double* Q, double* R, int nb, int nshards);

/* The same over `ngpu` REAL devices of this node ("qr_thin(..., int nb, int ngpu) ... owns its own threads /
 * RCCL communicator").  Device d (0 <= d < ngpu) factors the contiguous row block d of A on its own host thread; the R factors
 * travel in ONE ncclAllGather (librccl is dlopen()ed on the first call with ngpu > 1, never linked), every device factors
 * the stacked (ngpu*n) x n matrix redundantly and forms its rows of Q.  ngpu = 1 needs no communicator and gives exactly
 * qr_thin(..., nshards = 1).  Returns QR_E_ARG when ngpu exceeds the visible devices or a shard would have fewer than n rows.
 * Q is m x n, R is n x n (host memory).  No reference counterpart (the reference is single-device, qr.cu:711,737). */
int qr_thin_mgpu(const double* A, int m, int n, double* Q, double* R, int nb, int ngpu);

/* Device-resident TSQR step, one rank per GPU (one process or one host thread each), for callers whose row shard already lives
 * in HBM -- the per-GPU step of BASELINE configs C4 / C5.  No reference counterpart (single-device, qr.cu:711,737).
 *   rank 0:      qr_tsqr_unique_id(id)            128 bytes; carry them to every rank (MPI_Bcast, a key-value store, a file)
 *   every rank:  hipSetDevice(local gpu); qr_tsqr_plan_create(&tp, id, nranks, rank, m_local, n, nb)     (collective)
 *   per matrix:  qr_tsqr_factor_dev(tp, dA_shard, lda, dR)      local QR -> ONE ncclAllGather of the n x n R factors ->
 *                                                               redundant QR of the stacked (nranks n) x n matrix -> dR (n x n, ld n)
 *                qr_tsqr_formq_dev(tp, dA_shard, lda, dQ, ldq)  optional: this rank's m_local x n rows of the thin Q
 * Stream-ordered: no stream is drained inside a step; in the default guard mode (qr_plan_set_guard_mode below) the host thread waits
 * once per full-width panel of a shard above 16384 rows for that panel's verdict word while its last pass still runs -- latch mode on
 * qr_tsqr_local_plan(tp) removes even that.  The stacked factorisation of one call overlaps the local factorisation
 * of the next (independent matrices).  qr_tsqr_sync() before results are read on another stream.  librccl.so is dlopen()ed
 * on first use.  nranks = 1 needs no id (NULL) and no communicator; there qr_tsqr_factor_dev writes R straight into dR and does NOT
 * refresh the send buffer of qr_tsqr_exchange_buffers (qr_tsqr_local_dev does, at any rank count).  qr_tsqr_plan_create_comm takes an ncclComm_t the caller
 * already owns (as void*; NULL = the caller exchanges the factors itself: qr_tsqr_local_dev, copy through
 * qr_tsqr_exchange_buffers -- send: this rank's n*n doubles, recv: nranks*n*n in rank order --, qr_tsqr_stacked_dev). */
typedef struct qr_tsqr_plan qr_tsqr_plan;
#define QR_TSQR_UNIQUE_ID_BYTES 128
int qr_tsqr_unique_id(void* id128);
int qr_tsqr_plan_create(qr_tsqr_plan** tp, const void* id128, int nranks, int rank, int m_local, int n, int nb);
int qr_tsqr_plan_create_comm(qr_tsqr_plan** tp, void* nccl_comm, int nranks, int rank, int m_local, int n, int nb);
int qr_tsqr_plan_destroy(qr_tsqr_plan* tp);
int qr_tsqr_factor_dev(qr_tsqr_plan* tp, double* dA_shard, int lda, double* dR);
int qr_tsqr_formq_dev(qr_tsqr_plan* tp, const double* dA_shard, int lda, double* dQ, int ldq);
int qr_tsqr_local_dev(qr_tsqr_plan* tp, double* dA_shard, int lda);
int qr_tsqr_exchange_buffers(qr_tsqr_plan* tp, double** send, double** recv);
int qr_tsqr_stacked_dev(qr_tsqr_plan* tp, double* dR);
/* How the exchange is scheduled.  For single-stream (tall-skinny) shapes whose n is a multiple of the block size, qr_tsqr_factor_dev
 * goes block column by block column ("panel-pipelined", qr_tsqr_is_pipelined() = 1): block column k of a rank's R is final as soon as
 * local panel k is factored, so it is gathered (n / nb small ncclAllGathers instead of one) and the stacked matrix is factored
 * left-looking on a second stream WHILE the local factorisation continues -- only the last block column's share of the stacked QR
 * (~0.4 ms of 1.2 at 8 x 512 columns) is added to the latency of the step.  MI355XQR_TSQR_PIPE=0: one collective after the local QR.
 * qr_tsqr_factor_virtual_dev: the same schedule over P plans of ONE device from one thread (plans from
 * qr_tsqr_plan_create_comm(.., NULL, ..); the gather is device copies) -- tests and single-device bring-up.
 * qr_tsqr_factor_selfgather_dev: one rank's complete step with its own factor copied into every rank slot: the launches, streams and
 * events of a real rank minus the network (latency measurements on one GPU). */
int qr_tsqr_is_pipelined(qr_tsqr_plan* tp);
/* The schedule chosen by the caller instead: mode 0 = one collective after the local factorisation, 1 = panel-pipelined (QR_E_ARG when the
 * plan's shape cannot run it), 2 = back to the library's rule.  COLLECTIVE in the sense that every rank must make the same call between the
 * same two factorisations (the two forms issue different collectives); drains the plan.  bench.py --gpus N uses it to time both forms. */
int qr_tsqr_set_schedule(qr_tsqr_plan* tp, int mode);
/* The exchange of the last pipelined qr_tsqr_factor_dev, from events on the stacked plan's stream (drains the plan's streams):
 * out5[0] = sum over the block columns of [stacked stream past its wait for the local panel -> gather done] in ms, out5[1] = the longest
 * of them, out5[2] = the whole call, out5[3] = 1 pipelined / 0 one collective, out5[4] = 1 when the ranks fell back together.
 * With MI355XQR_TSQR_PIPE unset (or "auto") every rank contributes {out5[0], out5[2]} of its second call to one more all-gather before
 * its third and all apply the same rule: slowest rank's gathers > half of the fastest rank's step -> one collective from then on
 * (MI355XQR_TSQR_PIPE=1 keeps the pipelined form, =0 never uses it). */
int qr_tsqr_gather_stats(qr_tsqr_plan* tp, double* out5);
int qr_tsqr_factor_virtual_dev(qr_tsqr_plan** tps, int nranks, double** dA_shards, int lda, double** dR);
int qr_tsqr_factor_selfgather_dev(qr_tsqr_plan* tp, double* dA_shard, int lda, double* dR);
int qr_tsqr_sync(qr_tsqr_plan* tp);
void* qr_tsqr_stream(qr_tsqr_plan* tp);                 /* hipStream_t of the local step and the collective */
int qr_tsqr_comm_ranks(qr_tsqr_plan* tp, int* nranks);  /* ranks as RCCL itself counts them */

/* The host-pointer entry points (mmqr, explicitQR) keep their last few plans and device buffers, keyed by (device, m, n, nb),
 * so that repeated calls on same-sized matrices -- what the reference's harness does, qr.cu:776-789 -- do not pay ~10 ms of
 * allocation and stream creation each time.  This frees them (idle ones); MI355XQR_PLAN_CACHE=0 disables the cache. */
int qr_release_cached_plans(void);

/* ---------------------------------------------------------------------------------------------
 * 2. Device-resident API (all d* pointers are device memory of the current HIP device)
 * ------------------------------------------------------------------------------------------- */
typedef struct qr_plan qr_plan;

/* Workspace + streams for factoring matrices up to m x n with outer block nb and leaf width ib
 * (nb = 0 / ib = 0 select the library defaults).  A plan whose height is not a multiple of 16 (from 512 rows on, up to 4 GiB of
 * matrix) also holds an m x n buffer: qr_geqrf_dev at the plan's full height factors a copy of the caller's matrix with zero rows
 * appended -- same R, tau and V -- because an odd height or leading dimension keeps every kernel off its aligned path (x3). */
int qr_plan_create(qr_plan** plan, int m, int n, int nb, int ib);
int qr_plan_destroy(qr_plan* plan);

/* In-place blocked Householder QR of dA (m x n, lda), m <= plan m, n <= plan n; dtau: n doubles.
 * Device-side counterpart of mmqr (qr.c:55) with input already resident in HBM; asynchronous on the
 * plan's stream -- call qr_plan_sync before reading results on another stream.  The plan's streams are
 * non-blocking streams of their own: work queued on ANOTHER stream that writes a buffer handed to the plan
 * (a memset, a fill, a framework's allocation-time zeroing) must have completed -- synchronise that stream,
 * or make qr_plan_stream() wait on an event -- before the call, or it may land on top of the plan's output. */
int qr_geqrf_dev(qr_plan* plan, double* dA, int m, int n, int lda, double* dtau);

/* dC (m x ccols, ldc) <- Q * dC where Q = H_0..H_{n-1} comes from qr_geqrf_dev's factors.
 * identity_start != 0 first sets dC = I(m, ccols) and skips the structurally-zero part, i.e. forms
 * the leading ccols columns of Q (ccols = n: thin Q; ccols = m: the reference's m x m Q, qr.c:330). */
int qr_applyq_dev(qr_plan* plan, const double* dA, int m, int n, int lda, const double* dtau, double* dC,
                  int ccols, int ldc, int identity_start);

/* dR (rrows x n, ldr) = upper triangle of the factored dA, zero elsewhere (qr.c:334-343). */
int qr_extract_r_dev(qr_plan* plan, const double* dA, int m, int n, int lda, double* dR, int rrows, int ldr);

/* C = beta*C + alpha*op(A)*B with op = none ('N') or transpose ('T'); MFMA f64 tiles. */
int qr_gemm_dev(qr_plan* plan, char transa, int M, int N, int K, double alpha, const double* dA, int lda,
                const double* dB, int ldb, double beta, double* dC, int ldc);

/* Synthetic input: uniform[0,1) by a counter-based hash of the global element index, so any row
 * shard (rows [row_off, row_off+rows) of a total_rows x cols matrix) of the same seed is the same
 * data regardless of how many GPUs hold it.  Same distribution as the reference's
 * generator (qr.c:468-474), which is serial glibc rand() and kept for the small CPU-parity cases. */
int qr_fill_uniform_dev(qr_plan* plan, double* dA, int lda, long long rows, int cols, long long row_off,
                        long long total_rows, unsigned long long seed);
double qr_uniform_at(unsigned long long seed, unsigned long long linear_index);

/* sums[0] = ||X - Y||_F^2, sums[1] = ||Y||_F^2 over an rows x cols block.  Y is dY (ldy) if non-null,
 * else the generator above (row_off/total_rows/seed), else (mode 1) the identity.  Synchronous. */
int qr_diffnorm_dev(qr_plan* plan, const double* dX, int ldx, const double* dY, int ldy, long long rows,
                    int cols, long long row_off, long long total_rows, unsigned long long seed, int mode,
                    double* sums);

/* Device memory helpers so that a caller in any host language can use the device API without binding HIP itself
 * (the buffers are ordinary hipMalloc memory of the current device; copies are synchronous). */
int qr_device_malloc(void** dptr, size_t bytes);
int qr_device_free(void* dptr);
int qr_copy_to_device(void* dst, const void* src, size_t bytes);
int qr_copy_to_host(void* dst, const void* src, size_t bytes);

/* the two qr_plans inside a TSQR plan (profiling, fills, norms on the same streams); stacked: NULL when nranks = 1 */
qr_plan* qr_tsqr_local_plan(qr_tsqr_plan* tp);
qr_plan* qr_tsqr_stacked_plan(qr_tsqr_plan* tp);

/* Waits for everything queued on the plan's streams and reads the status words the panel kernels left on the device: QR_E_STALL /
 * QR_E_REFUSED (above) report a factorisation issued since the last call that must not be used; both are cleared by the call. */
int qr_plan_sync(qr_plan* plan);
/* What happens when the device-side guard refuses a full-width tall panel (>= MI355XQR_CQR_MIN_ROWS rows x 128 columns: CholeskyQR2 at
 * panel width needs cond(panel) < ~1e7 and full rank; no reference counterpart, the reference factors column by column, qr.c:109-235):
 *   latch = 0 (default): the panel is handed to the Householder-guarded leaf chain, the result is as good as for any other input.  The
 *              host thread reads the verdict from a host word the deciding kernel writes while the panel's last pass still runs: the GPU
 *              does not idle, but qr_geqrf_dev waits for that word once per tall panel (it is not capturable into a graph);
 *   latch = 1: qr_geqrf_dev never waits for the device (fully stream-ordered).  A refused panel makes the factorisation INVALID (the
 *              matrix is overwritten with garbage from that panel on); qr_plan_sync / qr_tsqr_sync return QR_E_REFUSED and the caller
 *              factors a fresh copy with latch = 0.  For pipelines that own their inputs and check a residual anyway.
 * MI355XQR_GUARD=latch selects latch = 1 for every plan a caller of the DEVICE API creates; the host-pointer entry points (mmqr, explicitQR,
 * qr_thin, qr_thin_mgpu) block anyway and always use latch = 0 on their own plans.
 * The call drains the plan and returns qr_plan_sync's status: a refusal latched before the switch is reported here, not lost. */
int qr_plan_set_guard_mode(qr_plan* plan, int latch);
/* out4: full-width tall panels issued, of them refused, leaves of one-launch panels that took their Householder route, one-launch
 * panels whose hand-off stalled -- since the plan was created (refusals in latch mode and the last two are counted at qr_plan_sync) */
int qr_plan_route_stats(qr_plan* plan, long long* out4);
/* out2: refused full-width panels that were retried PRECONDITIONED (shifted CholeskyQR3: R0 = chol(A^T A + s I), the same three-pass pipeline
 * on A R0^-1; default guard mode only), and how many of those the guard then accepted -- the others (rank deficient, cond > ~1e10) went
 * to the Householder leaf chain.  No reference counterpart (the reference factors column by column, qr.c:109-235). */
int qr_plan_retry_stats(qr_plan* plan, long long* out2);
void* qr_plan_stream(qr_plan* plan);          /* the hipStream_t work is queued on */
int qr_plan_update_cus(qr_plan* plan);        /* compute units the wide trailing update runs on (its share of the CU partition) */

/* Per-kernel-class timing with HIP events recorded on the plan's stream inside the timed region.
 * class 0 = trailing update A2 -= V*W (gemm_nn), 1 = W = (V T)^T A2 (gemm_tn + slab reduce),
 * 2 = panel factorisation (leaf kernels + in-panel updates + T), 3 = V*T and misc. */
#define QR_PROF_CLASSES 4
typedef struct qr_profile {
    double ms[QR_PROF_CLASSES];      /* summed event-to-event time */
    double flops[QR_PROF_CLASSES];   /* algorithmic flops issued */
    double bytes[QR_PROF_CLASSES];   /* algorithmic HBM bytes (compulsory traffic) */
    long long launches[QR_PROF_CLASSES];
} qr_profile;
/* on = 0: off; 1: every class; 2 * mask: only the classes whose bit is set in mask (bit c = class c; bits 4, 5 = the look-ahead
 * update / the panel stream's share of a wide update).  A record costs two event packets on its stream: profile what you read. */
int qr_plan_set_profile(qr_plan* plan, int on);
int qr_plan_pause_profile(qr_plan* plan, int pause);       /* stop / resume recording, keeping the records made so far */
/* what the plan was built with: outer / leaf block size, 1 = two-stream look-ahead schedule (any pointer may be NULL) */
int qr_plan_info(qr_plan* plan, int* nb, int* ib, int* lookahead);
int qr_plan_get_profile(qr_plan* plan, qr_profile* out);   /* synchronises, sums, resets */
/* The individual records behind the sums, in issue order (call before qr_plan_get_profile): class as above, plus 4 = the
 * look-ahead update of the next panel's columns and 5 = the panel stream's share of a wide update (both summed into class 3
 * by qr_plan_get_profile); start / end in ms since the first record began.  Returns the number of records written (<= max). */
int qr_plan_get_profile_records(qr_plan* plan, int max, int* cls, double* t0_ms, double* t1_ms);

/* Device facts + micro-probes used by bench.py / DESIGN.md (measured, not datasheet). */
int qr_device_info(char* arch, int arch_len, int* compute_units, int* clock_khz, size_t* hbm_bytes);
/* out3[0] = sustained back-to-back v_mfma_f64_16x16x4_f64 TFLOP/s (best over 1/2/4 workgroups per CU),
 * out3[1] = in-kernel shader clock (GHz) during that run, out3[2] = f64 VALU FMA TFLOP/s */
int qr_probe_mfma_f64_tflops(double* out3);
int qr_probe_copy_gbps(double* gbps);

/* ---------------------------------------------------------------------------------------------
 * 3. Solving with the factors: full-rank least squares min ||A X - B||, m >= n, fp64, column-major.
 * No reference counterpart (the reference stops at Q and R, qr.c:330-438); the LAPACK routine each call corresponds to is named.
 * Conventions of section 2: status return, queued on the plan's stream with no host wait, bad arguments (NULL plan or pointer, m < n,
 * nrhs < 1, ld* < rows, sizes above the plan's, an unknown trans) return QR_E_ARG before anything touches a device.  The device calls
 * do not look at R's diagonal: an exactly singular R gives inf / NaN in X.
 * Workspace for the right-hand sides grows lazily with nrhs (as qr_applyq_dev's does): the first call at a larger nrhs allocates,
 * and an allocation drains the plan and synchronises the device.
 * ------------------------------------------------------------------------------------------- */

/* LAPACK dlarft per outer block (dgeqrt's T layout): dT is nbp x n (ldt >= nbp, nbp = the plan's nb, qr_plan_info); columns [k, k+w)
 * hold the w x w upper-triangular T of reflectors k .. k+w-1 (zeros below its diagonal), so that H_k .. H_{k+w-1} = I - V T V^T.
 * Build once, apply many times. */
int qr_build_t_dev(qr_plan* plan, const double* dA, int m, int n, int lda, const double* dtau, double* dT, int ldt);

/* LAPACK dormqr (side 'L'): dC (m x nrhs, ldc) <- Q^T dC (trans 'T') or Q dC ('N'), Q = H_0 .. H_{n-1} from qr_geqrf_dev's factors.
 * V is read in place from dA (unit diagonal implied, upper triangle ignored).  dT from qr_build_t_dev, or NULL: T is rebuilt panel
 * by panel.  Up to 4 right-hand sides on tall matrices (m >= 16 n) a route of its own streams V twice per panel in place (no copy of V,
 * fixed-order sums); otherwise the MFMA products of qr_applyq_dev.  Either way repeated calls give bitwise-equal results. */
int qr_ormqr_dev(qr_plan* plan, char trans, const double* dA, int m, int n, int lda, const double* dtau, const double* dT, int ldt,
                 double* dC, int nrhs, int ldc);

/* LAPACK dtrtrs ('U', 'N', 'N'): dB (n x nrhs, ldb) <- R^{-1} dB, R = the upper triangle of the first n rows of the factored dA
 * (non-unit diagonal; n <= the plan's n).  Blocked back substitution: 64-row diagonal blocks by substitution (no inverse is formed),
 * one launch per block up to 64 right-hand sides, recursive halving with MFMA products above. */
int qr_solve_r_dev(qr_plan* plan, const double* dA, int n, int lda, double* dB, int nrhs, int ldb);

/* LAPACK dgels ('N', m >= n) on the device: factors dA in place (dtau: n doubles), overwrites dB (m x nrhs, ldb): rows 0..n-1 = X,
 * rows n..m-1 = the last m-n entries of Q^T B, so ||dB[n:m, j]|| is the residual norm of column j. */
int qr_gels_dev(qr_plan* plan, double* dA, int m, int n, int lda, double* dtau, double* dB, int nrhs, int ldb);

/* LAPACK dgels on host pointers, A (m x n) and B (m x nrhs) untouched: X (n x nrhs, ld n), resid (nrhs doubles, may be NULL) =
 * ||A x_j - b_j||_2 (from Q^T b_j).  Uses the plan cache of mmqr (qr_release_cached_plans).  Synchronous.  QR_E_SINGULAR when some
 * R(i,i) == 0 exactly (LAPACK dgels INFO > 0); X and resid hold no solution then. */
int qr_lstsq(const double* A, int m, int n, const double* B, int nrhs, double* X, double* resid);

/* ---------------------------------------------------------------------------------------------
 * 4. Column pivoting and rank: A P = Q R with |R(0,0)| >= |R(1,1)| >= ..., the numerical rank, and least squares for matrices whose
 * columns are dependent or nearly so (what section 3 cannot answer).  No reference counterpart (the reference stops at Q and R,
 * qr.c:330-438); the LAPACK routine each call corresponds to is named.  Conventions of sections 2 and 3: status return, work queued on
 * the plan's stream, bad arguments (NULL plan or pointer, m < n, n < 1, nrhs < 1, ld* < rows, sizes above the plan's) return QR_E_ARG
 * before anything touches a device.  Workspace hangs off the plan and is allocated on the first pivoted call (that call drains the plan).
 * Half of the work of a pivoted factorisation is one matrix-vector product with the whole trailing matrix per column (memory-bound):
 * measured: 11 to 25 times the cost of qr_geqrf_dev (README, "Pivoted QR").
 * ------------------------------------------------------------------------------------------- */

/* LAPACK dgeqp3 with every column free: A P = Q R.  dA (m x n, lda, m >= n) is overwritten exactly as qr_geqrf_dev overwrites it (R above,
 * reflector tails below with an implied unit diagonal, dtau: n doubles), so qr_applyq_dev, qr_build_t_dev, qr_ormqr_dev, qr_solve_r_dev
 * and qr_extract_r_dev work on the result unchanged.  djpvt: n ints on the device, 0-based: column j of A P is column djpvt[j] of the
 * caller's A.  At step j the pivot is the remaining column of largest partial norm, lowest index on a tie; partial norms are downdated
 * with LAPACK's safeguard (dlaqps), so a pivot can miss the true maximum by a relative sqrt(eps).
 * Stream-ordered inside a panel of 32 columns; the host thread waits for the device once per panel (it reads how many columns the
 * panel factored: a norm that has to be recomputed ends a panel early).  Repeated calls give bitwise-equal results. */
int qr_geqp3_dev(qr_plan* plan, double* dA, int m, int n, int lda, int* djpvt, double* dtau);

/* Numerical rank from the factors of qr_geqp3_dev: the number of i with |R(i,i)| > rcond * |R(0,0)|; rcond < 0 selects max(m, n) * DBL_EPSILON
 * (m = the height that was factored).  Synchronous (drains the plan's streams, reads n doubles back).  A zero matrix has rank 0. */
int qr_rank_dev(qr_plan* plan, const double* dA, int m, int n, int lda, double rcond, int* rank);

/* Rank-deficient least squares, basic solution (what MATLAB's backslash returns; NOT the minimum-norm solution of LAPACK dgelsy):
 * factors dA with pivoting, r = rank as above, X(djpvt[0..r), :) = R11^{-1} (Q^T B)(0..r, :), every other row of X = 0.
 * On return rows 0..n-1 of dB (m x nrhs, ldb) hold X in the caller's column order; rows n..m-1 hold the last m-n entries of Q^T B as in
 * qr_gels_dev; dresid (nrhs doubles on the device, may be NULL) = ||(Q^T b_j)(r..m)||_2 = ||A x_j - b_j||_2; *rank (host, may be NULL) = r.
 * Waits for the device as qr_geqp3_dev does and once more to read r; everything else is stream-ordered. */
int qr_gelsp_dev(qr_plan* plan, double* dA, int m, int n, int lda, int* djpvt, double* dtau, double* dB, int nrhs, int ldb,
                 double rcond, double* dresid, int* rank);

/* The same on host pointers, A (m x n) and B (m x nrhs) untouched (cf. qr_lstsq): X (n x nrhs, ld n), resid (nrhs doubles, may be NULL),
 * rank (may be NULL), jpvt (n ints, may be NULL).  Never returns QR_E_SINGULAR: a zero matrix gives rank 0 and X = 0.  Uses the plan
 * cache of mmqr (qr_release_cached_plans).  Synchronous. */
int qr_lstsq_pivoted(const double* A, int m, int n, const double* B, int nrhs, double rcond, double* X, double* resid, int* rank, int* jpvt);

/* ---------------------------------------------------------------------------------------------
 * 5. Minimum-norm solutions: underdetermined and transposed systems.  With A = Q R (m x n, m >= n, full rank) the system A^T X = B has
 * infinitely many solutions when m > n; the one of least norm is X = Q [R^{-T} B ; 0].  A wide system is the same thing read the other
 * way: factor its transpose.  No reference counterpart (the reference stops at Q and R, qr.c:330-438); the LAPACK routine each call
 * corresponds to is named.  Conventions of sections 2 to 4: status return, work queued on the plan's stream with no host wait, bad
 * arguments (NULL plan or pointer, nrhs < 1, ld* < rows, sizes above the plan's, the wrong one of m < n / m > n) return QR_E_ARG before
 * anything touches a device; the device calls do not look at R's diagonal (an exactly singular R gives inf / NaN in X); repeated calls
 * give bitwise-equal results (fixed-order sums, no floating-point atomics).  The entry points of section 3 keep answering QR_E_ARG
 * for m < n: everything here is a symbol of its own.
 * ------------------------------------------------------------------------------------------- */

/* LAPACK dtrtrs ('U', 'T', 'N'): dB (n x nrhs, ldb) <- R^{-T} dB, R = the upper triangle of the first n rows of the factored dA
 * (non-unit diagonal; n <= the plan's n).  Blocked forward substitution, the mirror of qr_solve_r_dev: 64-row diagonal blocks by
 * substitution (no inverse is formed), one launch per block up to 64 right-hand sides -- the launch updates every row below the block
 * just solved and solves the next one --, recursive halving with MFMA products above. */
int qr_solve_rt_dev(qr_plan* plan, const double* dA, int n, int lda, double* dB, int nrhs, int ldb);

/* Minimum-norm solution of A^T X = B from factors that already exist (qr_geqrf_dev's or qr_geqp3_dev's layout; for the latter the
 * system solved is (A P)^T X = B): factor once, solve many.  dB is m x nrhs (ldb >= m): rows 0..n-1 hold B on entry, rows n..m-1 are
 * ignored; on return dB = X = Q [R^{-T} B ; 0].  dT from qr_build_t_dev, or NULL, as in qr_ormqr_dev.  LAPACK: the dtrtrs + dormqr
 * half of dgels ('T'). */
int qr_minnorm_dev(qr_plan* plan, const double* dA, int m, int n, int lda, const double* dtau, const double* dT, int ldt, double* dB,
                   int nrhs, int ldb);

/* LAPACK dgels ('T', m >= n) on the device: factors dA in place (dtau: n doubles), then qr_minnorm_dev: dB (m x nrhs, ldb), rows
 * 0..n-1 = B on entry, = the minimum-norm X of A^T X = B on return. */
int qr_gels_t_dev(qr_plan* plan, double* dA, int m, int n, int lda, double* dtau, double* dB, int nrhs, int ldb);

/* dD (cols x rows, ldd >= cols) = dS (rows x cols, lds >= rows)^T, out of place, any sizes (not bounded by the plan's), leading
 * dimensions and bases; nothing outside the cols x rows block of dD is written.  64 x 64 tiles through LDS: the read and the write are
 * both contiguous.  No LAPACK counterpart (BLAS extensions call it omatcopy 'T'). */
int qr_transpose_dev(qr_plan* plan, const double* dS, int rows, int cols, int lds, double* dD, int ldd);

/* LAPACK dgels ('N', m <= n) for a wide column-major dA (m x n, lda >= m), which is not modified: the minimum-norm X of A X = B.
 * The plan is one for the TRANSPOSED shape: plan rows >= n, plan columns >= m.  dF (n x m, ldf >= n) receives the factors of A^T in
 * qr_geqrf_dev's layout and dtau its m scalars, so that qr_minnorm_dev(plan, dF, n, m, ldf, dtau, ..) solves again.  dB is n x nrhs
 * (ldb >= n): rows 0..m-1 hold B on entry; on return it holds X. */
int qr_gels_wide_dev(qr_plan* plan, const double* dA, int m, int n, int lda, double* dF, int ldf, double* dtau, double* dB, int nrhs,
                     int ldb);

/* LAPACK dgels ('N', m <= n) on host pointers, A (m x n) and B (m x nrhs, ld m) untouched: X (n x nrhs, ld n) = the minimum-norm
 * solution.  A is uploaded as it is and transposed on the device.  Uses the plan cache of mmqr, keyed on the transposed shape
 * (qr_release_cached_plans).  Synchronous.  QR_E_SINGULAR when some R(i,i) == 0 exactly (X holds no solution then); QR_E_ARG when m > n. */
int qr_lstsq_minnorm(const double* A, int m, int n, const double* B, int nrhs, double* X);

/* ---------------------------------------------------------------------------------------------
 * 6. Row-append updating and streaming least squares: rows that arrive in pieces.  The building block is the QR factorisation of a
 * triangle stacked on a block of new rows, [R ; B] = Q' [R' ; 0] -- the step TSQR is made of --, which costs 2 p n^2 flops for p new
 * rows instead of the 2 (n + p) n^2 of a dense factorisation of the stacked matrix, never touches the zero half of R and works for any
 * p >= 1.  No reference counterpart (the reference factors one resident matrix, qr.c:55-313); the LAPACK routine each call corresponds
 * to is named.  Conventions of sections 2 to 5: status return, work queued on the plan's stream with no host wait unless stated
 * otherwise, bad arguments (NULL plan or pointer, a size below 1 or above its limit, ld* < rows, an unknown trans) return QR_E_ARG
 * before anything touches a device; repeated calls give bitwise-equal results (fixed-order sums, no floating-point atomics); fp64,
 * column-major.
 * ------------------------------------------------------------------------------------------- */

/* Reflectors are blocked in panels of QR_TPQRT_PANEL columns (a constant of the implementation); a block of new rows handed to one
 * call has at most qr_tpqrt_max_rows() = 256 rows: the update kernel keeps the 256 x 32 reflector panel AND a 256 x 32 slab of the
 * matrix it updates in one workgroup's LDS (2 x 64.5 KiB, + 25 KiB of T and W tiles, of the CU's 160 KiB), so that the slab is read
 * from memory once and written once; 512 rows would leave no room for the slab.  Taller blocks go through the accumulator below or are
 * fed block by block: qr_tpqrt_dev answers QR_E_ARG above the limit. */
#define QR_TPQRT_PANEL 32
int qr_tpqrt_max_rows(void);

/* LAPACK dtpqrt (M = p, N = n, L = 0).  On entry dR (ldr >= n) is n x n upper triangular -- its strict lower triangle is neither read
 * nor written -- and dB (ldb >= p) is p x n, 1 <= p <= qr_tpqrt_max_rows(), n <= the plan's n.  On return dR holds R' with
 * [R ; B] = Q' [R' ; 0], dB holds V: reflector j is [e_j ; V(:, j)], the identity on top is implied; dT (QR_TPQRT_PANEL x n,
 * ldt >= QR_TPQRT_PANEL) is the block T in qr_build_t_dev's layout at a panel width of QR_TPQRT_PANEL: columns [k, k + w) hold the
 * w x w upper-triangular T of reflectors k .. k + w - 1, zeros below its diagonal.
 * LAPACK dlarfg per column: beta = -sign(R(j,j)) hypot(R(j,j), |B(:,j)|); a column of B that is exactly zero gives tau = 0 and leaves
 * everything untouched, so R = 0 on entry is legal (that is how an accumulation starts); exact zeros in B stay exact zeros, so a caller
 * may hand over an upper-triangular block with explicit zeros and get V of the same shape.  (dlarfg's rescaling of subnormal columns
 * is not reproduced.  Tested range, this section and 6b: bitwise equivariant under scaling [R ; B] by 2^-299 .. 2^301, and at 2^+-480
 * -- entries of about 1e+-144 -- the Gram identity holds as for entries of order one, tests/test_gpu_range_edges.py.)  Two launches per QR_TPQRT_PANEL columns. */
int qr_tpqrt_dev(qr_plan* plan, double* dR, int n, int ldr, double* dB, int p, int ldb, double* dT, int ldt);

/* LAPACK dtpmqrt (side 'L', L = 0): [C1 ; C2] <- Q'^T [C1 ; C2] (trans 'T') or Q' [C1 ; C2] ('N') with dV, dT from qr_tpqrt_dev;
 * dC1 is n x nrhs (ldc1 >= n), dC2 is p x nrhs (ldc2 >= p).  One launch per panel. */
int qr_tpmqrt_dev(qr_plan* plan, char trans, const double* dV, int p, int n, int ldv, const double* dT, int ldt,
                  double* dC1, int ldc1, double* dC2, int ldc2, int nrhs);

/* Least-squares accumulator for min ||A x_j - b_j|| over rows that arrive chunk by chunk: it keeps R (n x n), Z = the first n entries
 * of Q^T b (n x nrhs) and one sum of squares per right-hand side, all zero at the start; n <= the plan's n.  The plan must outlive it.
 *   qr_lsacc_push_dev    folds in p >= 1 rows [dA | dB] (dA: p x n, lda >= p; dB: p x nrhs, ldb >= p) and uses both buffers as workspace:
 *                        they hold nothing defined on return.  The route follows from the shape by construction, not from a measured rule:
 *                          p >= n (p <= the plan's m): qr_geqrf_dev on the chunk, qr_ormqr_dev('T') on its right-hand sides, rows n .. p
 *                             of the result into the sums of squares, then the chunk's triangle is merged in row blocks of at most
 *                             qr_tpqrt_max_rows() rows: block i of an upper-triangular matrix is zero left of column i * rows, so its
 *                             merge works on R[i rows:, i rows:] only -- the zero columns are skipped, not multiplied;
 *                          p < n: qr_tpqrt_dev directly on the rows, in row blocks of at most qr_tpqrt_max_rows(), one after the other.
 *                        In both routes the right-hand sides ride along (qr_tpmqrt_dev 'T'), and what is left in their new rows goes
 *                        into the sums of squares.
 *   qr_lsacc_rows        rows pushed so far (host bookkeeping, no device access)
 *   qr_lsacc_factor_dev  the device addresses of R (upper triangular, zeros below) and Z and their leading dimensions (any may be NULL);
 *                        they stay valid, and change with every push, until the accumulator is destroyed
 *   qr_lsacc_solve_dev   dX (n x nrhs, ldx >= n) = R^{-1} Z through qr_solve_r_dev; dresid (nrhs doubles on the device, may be NULL) =
 *                        the square roots of the sums of squares = ||A x_j - b_j||_2.  The state is untouched: pushing may continue.
 *                        Like qr_gels_dev it does not look at R's diagonal.
 *   qr_lsacc_reset       back to the empty state;  qr_lsacc_destroy waits for the plan's stream, then frees. */
typedef struct qr_lsacc qr_lsacc;
int qr_lsacc_create(qr_lsacc** acc, qr_plan* plan, int n, int nrhs);
int qr_lsacc_push_dev(qr_lsacc* acc, double* dA, int p, int lda, double* dB, int ldb);
int qr_lsacc_rows(qr_lsacc* acc, long long* rows);
int qr_lsacc_factor_dev(qr_lsacc* acc, const double** dR, int* ldr, const double** dZ, int* ldz);
int qr_lsacc_solve_dev(qr_lsacc* acc, double* dX, int ldx, double* dresid);
int qr_lsacc_reset(qr_lsacc* acc);
int qr_lsacc_destroy(qr_lsacc* acc);

/* Least squares on host pointers for a matrix taller than the device should hold: A (m x n, lda >= m) and B (m x nrhs, ldb >= m) are
 * untouched; chunk_rows rows at a time (at most m) are uploaded and pushed into an accumulator, so device memory is bounded by the
 * chunk, not by m.  X (n x nrhs, ld n), resid (nrhs doubles, may be NULL) as in qr_lstsq.  Uses the plan cache of mmqr, keyed on
 * (max(chunk_rows, n), n) (qr_release_cached_plans).  Synchronous.  QR_E_SINGULAR when some R(i,i) == 0 exactly, and when m < n
 * (X holds no solution then); QR_E_ARG for chunk_rows < 1. */
int qr_lstsq_chunked(const double* A, long long m, int n, int lda, const double* B, int nrhs, int ldb,
                     int chunk_rows, double* X, double* resid);

/* ---------------------------------------------------------------------------------------------
 * 6b. Row removal: the signed-row update of R and sliding-window least squares.  Section 6 can only add rows; here the last p_del rows
 * of a block are REMOVED while its first p_add rows are added, in one pass: with S = diag(+1 .. +1, -1 .. -1) over the block's rows,
 * R' is the upper triangle with R'^T R' = R^T R + B^T S B.  The transformation is a product of hyperbolic Householder reflectors
 * Theta_j = I - tau_j u_j u_j^T Phi, u_j = [e_j ; v_j], Phi = diag(I_n, S), tau_j (1 + v_j^T S v_j) = 2, which keep the signed Gram
 * matrix [R ; B]^T Phi [R ; B]; per column dlarfg's formulas hold with every inner product over the block's rows weighted by S:
 * d = R(j,j)^2 + b^T S b, beta = -sign(R(j,j)) sqrt(d), v = b / (R(j,j) - beta), tau = (beta - R(j,j)) / beta.  d is formed without
 * cancellation as (h - |b_del|)(h + |b_del|), h = hypot(R(j,j), |b_add|).  A panel of QR_TPQRT_PANEL columns is I - U T U^T Phi with
 * the compact-WY recursion of section 6 on V^T S V.  No reference counterpart; no LAPACK one either (LINPACK dchdd removes one row with
 * plane rotations).  Conventions of section 6: status return, bad arguments return QR_E_ARG before anything touches a device, fixed-order
 * sums, bitwise-equal repeats, fp64, column-major; the same row limit, now on p_add + p_del.
 * Failure: a column with d <= 0, or d not finite, means that the rows to be removed are not contained in the matrix R belongs to (or
 * that too few rows would be left): there is no positive-definite R'.  The kernel that meets it writes the column + 1 into a device
 * word that hangs off the plan and stops; every later launch of the same call reads the word first and returns at once; the host reads
 * it once, at the end of the call: QR_E_NOTPD.
 * Stability: the method is NOT backward stable in the sense the orthogonal update is.  Its error grows with ||R R'^{-1}||, the
 * conditioning of the removal itself: removing rows that carry most of a column's mass loses that many digits, as it must -- the
 * triangle no longer holds the information.  A removal that leaves a well-conditioned R' from a well-conditioned R is as accurate as
 * the update (the Gram identity to n eps in the tests).  Adding and removing in one pass keeps d further from zero than removing first.
 * ------------------------------------------------------------------------------------------- */

/* qr_tpqrt_dev with signed rows: dB is (p_add + p_del) x n, its first p_add rows are added, its last p_del rows removed; p_add >= 0,
 * p_del >= 0, 1 <= p_add + p_del <= qr_tpqrt_max_rows(), ldb >= p_add + p_del.  dR, dB (<- V), dT as qr_tpqrt_dev.  An exactly zero
 * column of B: tau = 0, nothing touched.  The host thread waits once, at the end, and reads the status word: QR_E_NOTPD with *info
 * (host, may be NULL) = the failing column + 1 -- dR and dB are undefined then -- else 0 and *info = 0.  With p_del == 0 this IS
 * qr_tpqrt_dev (the same launches, bitwise the same result) followed by the wait.  Two launches per QR_TPQRT_PANEL columns. */
int qr_tphqrt_dev(qr_plan* plan, double* dR, int n, int ldr, double* dB, int p_add, int p_del, int ldb, double* dT, int ldt, int* info);

/* Applies to [C1 ; C2] (dC1: n x nrhs, ldc1 >= n; dC2: (p_add + p_del) x nrhs) the transformation that took [R ; B] to [R' ; 0], with
 * dV, dT from qr_tphqrt_dev: panel by panel W = T^T (C1 + V^T S C2), C1 -= W, C2 -= V W.  That one direction is what right-hand sides
 * need; it keeps |C1(:, c)|^2 + C2(:, c)^T S C2(:, c).  Stream-ordered, no host wait.  One launch per panel. */
int qr_tphmqrt_dev(qr_plan* plan, const double* dV, int p_add, int p_del, int n, int ldv, const double* dT, int ldt,
                   double* dC1, int ldc1, double* dC2, int ldc2, int nrhs);

/* The accumulator of section 6 with rows leaving:
 *   qr_lsacc_pop_dev    removes p >= 1 rows [dA | dB] that were pushed earlier (dA: p x n, lda >= p; dB: p x nrhs, ldb >= p; both
 *                       untouched), in blocks of at most qr_tpqrt_max_rows().  Z rides along; the sums of squares become rss - |E|^2, E =
 *                       what the transformation leaves in the removed rows of the right-hand sides, clamped at 0.
 *   qr_lsacc_slide_dev  adds pnew rows and removes pold rows in one pass: new stacked over old in the accumulator's workspace, in blocks
 *                       with p_add + p_del <= qr_tpqrt_max_rows().  The inputs are untouched.
 * Both are all-or-nothing: they work on copies of R, Z and the sums and commit them with device copies after the last block succeeded;
 * on QR_E_NOTPD the accumulator is bitwise what it was.  They wait once for the status word.  More rows removed than held: QR_E_ARG.
 * Fewer than n rows left -- removing every row included --: QR_E_NOTPD before any launch (no triangle of full rank can remain; to
 * start over use qr_lsacc_reset).  The workspace (a copy of R, Z and the sums, one block of qr_tpqrt_max_rows() rows) is allocated on the first call and freed by qr_lsacc_destroy. */
int qr_lsacc_pop_dev(qr_lsacc* acc, const double* dA, int p, int lda, const double* dB, int ldb);
int qr_lsacc_slide_dev(qr_lsacc* acc, const double* dAnew, int pnew, int ldan, const double* dBnew, int ldbn,
                       const double* dAold, int pold, int ldao, const double* dBold, int ldbo);

/* Least squares over a window that moves, on host pointers; A (m x n, lda >= m) and B (m x nrhs, ldb >= m) are untouched.  Window k is
 * rows [k step, k step + window), k = 0 .. (m - window) / step.  X: one n x nrhs solution (ld n) per window, one after the other;
 * resid: nrhs values per window, may be NULL.  The first window is pushed, each later one is ONE slide (step rows in, step rows out).
 * QR_E_ARG for window < n, step < 1, step > window, window > m; QR_E_SINGULAR as qr_lstsq_chunked (first window); QR_E_NOTPD when a
 * later window loses full rank.  Uses the plan cache of mmqr, keyed on (window, n).  Synchronous. */
int qr_lstsq_rolling(const double* A, long long m, int n, int lda, const double* B, int nrhs, int ldb, int window, int step,
                     double* X, double* resid);

/* ---------------------------------------------------------------------------------------------
 * 7. Singular values, SVD and minimum-norm least squares of rank-deficient systems.  With A = Q R (m x n, m >= n) and the SVD of the
 * n x n triangle, R = W S Z^T, A = (Q W) S Z^T: the tall part is qr_geqrf_dev, the small dense part a one-sided block Jacobi SVD (LAPACK
 * dgesvj; dgejsv takes the same QR-then-Jacobi route).  The iteration runs on R^T, not R: the rows of a triangular factor are far
 * closer to orthogonal than its columns (an n = 96 matrix of condition 1e10 took 4 sweeps on R^T against 15 on R in a CPU emulation of
 * this algorithm; dgejsv makes the same choice).  No reference counterpart (the reference stops at Q and R, qr.c:330-438); the LAPACK
 * routine each call corresponds to is named.  Conventions of sections 3 to 6: status return, work queued on the plan's stream, bad
 * arguments (NULL plan or pointer, sizes below 1 or above the plan's, ld* < rows, an unknown job letter) return QR_E_ARG before anything
 * touches a device; repeated calls give bitwise-equal results (fixed-order sums, exact maxima, no floating-point atomics); fp64,
 * column-major.  Workspace hangs off the plan and is allocated on the first call of this section (that call drains the plan).
 *
 * The iteration: the columns are cut into blocks of QR_JSVD_BLOCK; a sweep is a round-robin tournament over the blocks (below), one
 * launch per round, one workgroup per block pair: Gram matrix of the pair's 64 columns on MFMA tiles, cyclic Jacobi rotations of the
 * smaller angle on that 64 x 64 matrix in LDS, the accumulated 64 x 64 rotation applied to the columns on MFMA tiles.  A pair whose
 * columns are already orthogonal to tol = sqrt(rows) * DBL_EPSILON (LAPACK's threshold: max |g_i . g_j| / (|g_i| |g_j|)) is left alone;
 * the iteration ends with the first sweep in which every pair was (so an input with orthogonal columns takes one sweep, and the count
 * reported includes that last, idle sweep).  No workgroup waits for another; the sweep loop is bounded by QR_JSVD_MAX_SWEEPS on the host.
 * Accuracy is that of the QR itself: values to n eps of the largest, norm-wise.  Two columns whose norms differ by more than a factor
 * DBL_EPSILON are not rotated against each other (the smaller one cannot change the larger by an ulp): that is what lets an exactly
 * rank-deficient input converge, and it is why values below eps times their neighbours' carry no relative accuracy.  Column norms are plain sums of squares (dgesvj's
 * rescaling against over- and underflow is not reproduced).  Tested range: U, V, the sweep count and sigma / s are bitwise the same for
 * an input scaled by s = 2^-299 .. 2^301, and at s = 2^+-480 (entries of about 1e+-144) reconstruction and orthogonality stay within
 * sweeps * n * eps (tests/test_gpu_scale_equivariance.py, tests/test_gpu_range_edges.py); beyond that the squares leave the normal range.
 * Out of scope: m < n (transpose with qr_transpose_dev and swap the roles of U and V); a qr_geqp3_dev-preconditioned variant for high
 * RELATIVE accuracy of tiny singular values (dgejsv's); a multi-GPU driver (it follows from qr_tsqr_factor_dev's R and is a later change).
 * ------------------------------------------------------------------------------------------- */
#define QR_JSVD_BLOCK 32
#define QR_JSVD_MAX_SWEEPS 30      /* LAPACK dgesvj's limit */

/* The tournament the device code runs, on the host (no device is touched): nblk = ceil(n / QR_JSVD_BLOCK) column blocks, `rounds` rounds
 * per sweep -- nblk for an odd nblk (one block sits out each round), nblk - 1 for an even one; a sweep contains every unordered pair of
 * distinct blocks exactly once and no block twice in a round.  nblk == 1: one round with the self-pair (0, 0).
 * qr_jsvd_round_pairs writes round `round`'s pairs as 2 ints each (p, q), p < q, into pairs (room for cap pairs) and returns their
 * count; QR_E_ARG for n < 1, a round outside [0, rounds), NULL pairs or too small a cap.  (Circle method: with N = the odd one of
 * nblk, nblk - 1, round s pairs (s + k) mod N with (s - k) mod N, k = 1 .. (N - 1) / 2; an even nblk adds (s, nblk - 1).) */
int qr_jsvd_rounds(int n, int* nblk, int* rounds);
int qr_jsvd_round_pairs(int n, int round, int* pairs, int cap);

/* LAPACK dgesvj (r >= n; r <= the plan's m, n <= the plan's n).  On entry dG (ldg >= r) is any r x n matrix.  On return dS[0..n) holds
 * the singular values in descending order and the columns of dG the left singular vectors, of unit norm; a column whose singular value
 * is exactly 0 is an exact zero column.  jobv 'V': dV (n x n, ldv >= n) holds the right singular vectors, G_in = dG diag(dS) dV^T;
 * jobv 'N': dV may be NULL, no rotations are accumulated (dS is bitwise the same).  *sweeps (host, may be NULL) = sweeps used.
 * The host thread waits once per sweep (it reads the sweep's convergence word) and once more for the descending sort: n doubles come
 * back, n ints go out; the sort is stable, ties keep column order.  Everything else is stream-ordered.  QR_E_NOCONV after
 * QR_JSVD_MAX_SWEEPS sweeps.  Nothing outside the r x n / n x n / n extents is written. */
int qr_gesvj_dev(qr_plan* plan, char jobv, double* dG, int r, int n, int ldg, double* dS, double* dV, int ldv, int* sweeps);

/* The SVD of a tall matrix (LAPACK dgesvd / dgejsv with jobs 'S' / 'N'), m >= n: qr_geqrf_dev on dA (the factors stay in dA, dtau as
 * usual: qr_ormqr_dev etc. keep working on them), R^T into an n x n workspace, qr_gesvj_dev's iteration on it.  dS: n values, descending.
 * jobv 'V': dV (n x n, ldv >= n) = the right singular vectors of A (the normalised columns of the iterate); 'N': dV may be NULL.
 * jobu 'U': dU (m x n, ldu >= m) = Q [Z ; 0] with Z the accumulated rotations, through qr_ormqr_dev ('N'); 'N': dU may be NULL.
 * A = dU diag(dS) dV^T.  jobu = jobv = 'N': values only, no accumulation and no Q apply (dS is bitwise the same).  A column of dU
 * that belongs to a zero singular value is a unit vector orthogonal to the others, as in LAPACK.  Host waits as qr_gesvj_dev. */
int qr_gesvd_dev(qr_plan* plan, char jobu, char jobv, double* dA, int m, int n, int lda, double* dtau, double* dS, double* dU, int ldu,
                 double* dV, int ldv, int* sweeps);

/* 2-norm condition number sigma_max / sigma_min through the values-only path (dA is factored in place); inf when sigma_min == 0, and
 * whenever R(i,i) == 0 exactly for some i (qr_lstsq's test: an exactly zero column, for one -- R is then exactly singular, and the
 * iteration would return rounding noise in place of that zero).  Synchronous.  (LAPACK: dgesvd + a division; dtrcon estimates the 1-norm one.) */
int qr_cond_dev(qr_plan* plan, double* dA, int m, int n, int lda, double* dtau, double* cond);

/* LAPACK dgelss (m >= n): the minimum-norm solution of min ||A X - B|| for any rank -- what section 4's basic solution is not.  Factors
 * dA, applies Q^T to dB (m x nrhs, ldb >= m), runs the iteration on R^T = Y S Z^T with accumulation and forms X = Y S^+ (Z^T c),
 * c = (Q^T B)(0:n): S^+ inverts sigma_i > rcond * sigma_0 and zeroes the rest; rcond < 0 selects max(m, n) * DBL_EPSILON as qr_rank_dev
 * does.  On return rows 0..n-1 of dB hold X, rows n..m-1 are as qr_gels_dev leaves them; dS: the n singular values; *rank (host, may be
 * NULL) = the number of inverted values.  A zero matrix gives rank 0 and X = 0, not an error.  Host waits as qr_gesvj_dev. */
int qr_gelss_dev(qr_plan* plan, double* dA, int m, int n, int lda, double* dtau, double* dB, int nrhs, int ldb, double rcond, double* dS,
                 int* rank);

/* The tall SVD on host pointers, A (m x n, m >= n) untouched: S (n, descending), U (m x n, ld m) and V (n x n, ld n) may each be NULL.
 * Uses the plan cache of mmqr (qr_release_cached_plans).  Synchronous. */
int qr_svd(const double* A, int m, int n, double* S, double* U, double* V);

/* LAPACK dgelss on host pointers, A (m x n, m >= n) and B (m x nrhs) untouched: X (n x nrhs, ld n); resid (nrhs doubles, may be NULL) =
 * ||A x_j - b_j||_2, from the last m - n entries of Q^T b_j and the components along the discarded singular vectors; rank and S (n
 * doubles) may be NULL.  Uses the plan cache of mmqr.  Synchronous. */
int qr_lstsq_svd(const double* A, int m, int n, const double* B, int nrhs, double rcond, double* X, double* resid, int* rank, double* S);

/* ---------------------------------------------------------------------------------------------
 * 8. Batched factorisation and least squares of small matrices: many independent m x n problems (m >= n, n <= QR_BATCHED_MAX_N,
 * m within what n columns leave of the LDS, see qr_batched_max_rows) in one call -- per-series regressions, per-element fits, what rocSOLVER's geqrf_strided_batched and
 * torch.linalg.qr on a batch are used for.  Matrix q of a batch lives at base + q * stride; it is column-major and strides count doubles
 * (a packed batch: lda = m, strideA = m * n, stridetau = n).  No reference counterpart (the reference factors one matrix per call).
 *
 * The results follow LAPACK dgeqr2 / dlarfg exactly: beta = -sign(alpha) hypot(alpha, |x|), tau = (beta - alpha) / beta,
 * v = x / (alpha - beta); x == 0 exactly gives tau = 0 and leaves the column unchanged (so the last column of a square matrix has
 * tau = 0); R on and above the diagonal, V below it with an implicit unit diagonal.  R, V and tau agree with LAPACK's up to rounding,
 * signs included.
 *
 * One wave factors a matrix of m <= 64 rows and at most 32 columns in registers (four matrices per workgroup); anything larger is
 * factored by one workgroup with the matrix resident in LDS.  The route follows from the shape alone, never from `batch` or a matrix's
 * index, and every sum runs in a fixed order: repeated calls are bitwise equal, and a matrix's result is bitwise independent of the
 * batch count and of its position in the batch.  No atomics.
 *
 * The plan supplies the stream only: m and n of a call are not bound by the plan's shape.  Calls queue on the plan's stream and do not
 * wait on the host; geqrf and ormqr are one launch each, orgqr two, gels one or three (below), whatever `batch` is.  Bad arguments return
 * QR_E_ARG before anything touches a device: a NULL plan or pointer, m < n, n < 1, n > QR_BATCHED_MAX_N, an m that does not fit (below),
 * ld* < m, nrhs < 1, an unknown trans, a stride smaller than the block it steps over (strideA < lda * n, stridetau < n, strideC <
 * ldc * nrhs, ...), batch < 0.  batch == 0 returns 0 and launches nothing.
 * ------------------------------------------------------------------------------------------- */
#define QR_BATCHED_MAX_N 64

/* The rows the calls of this section are certain to take for ncols columns held in LDS: 512 for 1 <= ncols <= 32, 256 for
 * 33 <= ncols <= 64, 0 otherwise (160 KiB of LDS at a leading dimension of m + 2: 32 * 514 and 64 * 258 doubles, plus the small
 * arrays).  The value is that of the widest matrix of its class; a narrower one is taken while it fits: m <= 512 and n columns at the
 * leading dimension ld = the smallest value >= m that is 2 mod 32, n * ld + 72 doubles within 160 KiB (300 x 40 is taken, 300 x 64 is
 * not).  What does not fit is QR_E_ARG.  No device is touched. */
int qr_batched_max_rows(int ncols);

/* LAPACK dgeqr2 of every matrix in place: R and V over dA, tau (n per matrix) to dtau. */
int qr_geqrf_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                         double* dtau, long long stridetau, int batch);

/* LAPACK dormqr, side 'L': dC (m x nrhs per matrix, any nrhs >= 1) <- Q^T dC (trans 'T') or Q dC ('N') from the factors of
 * qr_geqrf_batched_dev. */
int qr_ormqr_batched_dev(qr_plan* plan, char trans, const double* dA, int m, int n, int lda, long long strideA,
                         const double* dtau, long long stridetau,
                         double* dC, int nrhs, int ldc, long long strideC, int batch);

/* LAPACK dorgqr: the thin m x n Q of every matrix into dQ (the identity written on the device, then ormqr 'N'). */
int qr_orgqr_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA,
                         const double* dtau, long long stridetau,
                         double* dQ, int ldq, long long strideQ, int batch);

/* LAPACK dgels ('N', m >= n) per matrix: dA is factored in place, dB (m x nrhs) receives X in rows 0..n-1; the sum of squares of rows
 * n..m-1 of a column is that column's residual sum of squares.  dinfo (batch device ints): 0, or i + 1 for the smallest i with
 * R(i,i) == 0 exactly; such a matrix's dB holds Q^T B and no solve is done for it, the others are unaffected, and the call still returns 0.
 * One fused launch when n + nrhs <= QR_BATCHED_MAX_N and m <= qr_batched_max_rows(n + nrhs): the right-hand sides ride along as extra
 * columns that are updated but never factored, and the back substitution runs in the same kernel (the route then follows from
 * (m, n + nrhs)).  Otherwise the composition geqrf, ormqr 'T', a batched back substitution. */
int qr_gels_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                        double* dtau, long long stridetau,
                        double* dB, int nrhs, int ldb, long long strideB, int* dinfo, int batch);

/* The thin QR of a packed batch on host pointers (A untouched; lda = m, stride = m * n): Q m x n and R n x n (zeros below the diagonal)
 * per matrix.  Creates a plan of its own.  Synchronous. */
int qr_thin_batched(const double* A, int m, int n, int batch, double* Q, double* R);

/* dgels on a packed batch on host pointers (A: m x n, B: m x nrhs per matrix, both untouched): X n x nrhs per matrix, resid (nrhs per
 * matrix, may be NULL) = ||A x_j - b_j||_2, info[batch] as dinfo above.  Returns QR_E_SINGULAR if any info entry is non-zero (X of such a
 * matrix holds no solution; the others are valid).  Synchronous. */
int qr_lstsq_batched(const double* A, int m, int n, const double* B, int nrhs, int batch,
                     double* X, double* resid, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8b. Batched column-pivoted QR and rank-deficient least squares: section 8 for batches in which some matrix may be rank-deficient (a
 * constant regressor, a duplicated feature, fewer distinct samples than unknowns).  Section 8's conventions hold unchanged: the layout
 * (base + q * stride, column-major, strides in elements: doubles for dA, dtau, dB, ints for djpvt), the shape limits
 * (n <= QR_BATCHED_MAX_N, m as qr_batched_max_rows describes), the plan that supplies the stream only, no host wait, QR_E_ARG for bad
 * arguments before anything touches a device (djpvt NULL, stridejpvt < n and a NaN rcond among them), batch == 0 returns 0, no atomics, every sum in
 * a fixed order, results bitwise repeatable and bitwise independent of `batch` and of a matrix's index.
 *
 * The factorisation is LAPACK dgeqp3 with every column free (its unblocked kernel dlaqp2) per matrix, A P = Q R: at step j the
 * remaining column of largest partial norm is swapped in, the lowest index on a tie; the partial norms are downdated by
 * vn1 *= sqrt(max(0, 1 - (|A(j,c)| / vn1)^2)) and recomputed from rows j+1..m-1 when that estimate times (vn1 / vn2)^2 is at most
 * sqrt(eps).  The matrix is in registers or LDS throughout, so norms, arg-max and swap never touch memory: one launch whatever `batch`
 * is.  The rank of a factored matrix is the length of the leading run of |R(i,i)| > rcond |R(0,0)|; rcond < 0 selects
 * max(m, n) * DBL_EPSILON; a zero matrix has rank 0.
 * ------------------------------------------------------------------------------------------- */

/* dgeqp3 of every matrix in place.  dA comes back in the layout of qr_geqrf_batched_dev (R, V, dlarfg signs, tau = 0 for a column with
 * nothing below it), so qr_ormqr_batched_dev and qr_orgqr_batched_dev apply to it unchanged.  djpvt: n ints per matrix, 0-based: column
 * j of A P is column djpvt[j] of the caller's matrix. */
int qr_geqp3_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                         int* djpvt, long long stridejpvt, double* dtau, long long stridetau, int batch);

/* drank[q] (batch device ints) = the rank of matrix q from the factors of qr_geqp3_batched_dev, written in stream order: unlike
 * qr_rank_dev this call does not wait for the device. */
int qr_rank_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA,
                        double rcond, int* drank, int batch);

/* Rank-deficient least squares per matrix: factor with pivoting, r = the rank as above, X into rows 0..n-1 of dB in the caller's column
 * order.  qr_gelsp_batched_dev gives the basic solution (section 4's meaning: X(jpvt[0..r), :) = R11^-1 (Q^T B)(0..r, :), every other row
 * exactly 0.0); qr_gelsy_batched_dev the minimum-norm one (LAPACK dgelsy, what numpy.linalg.lstsq returns): [R11 R12] = [T11 0] Z by r
 * reflectors from the right (dtzrzf), X = P Z^T [T11^-1 (Q^T B)(0..r, :); 0].  With r == n the two give the same bits.
 * Rows n..m-1 of dB hold the tail of Q^T B as in qr_gels_batched_dev; dresid (nrhs doubles per matrix, packed, may be NULL) =
 * ||(Q^T b_j)(r..m)||_2 = ||A x_j - b_j||_2; drank (batch ints, may be NULL) = r.  dA, dtau and djpvt come back as
 * qr_geqp3_batched_dev leaves them; Z is not returned.  Singularity is never an error: a zero matrix gives rank 0 and X = 0.
 * One fused launch when n + nrhs <= QR_BATCHED_MAX_N and m <= qr_batched_max_rows(n + nrhs) (the right-hand sides ride along as
 * columns that are updated but never pivoted or factored); otherwise geqp3, ormqr 'T' and a batched solve (three launches). */
int qr_gelsp_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                         int* djpvt, long long stridejpvt, double* dtau, long long stridetau,
                         double* dB, int nrhs, int ldb, long long strideB,
                         double rcond, double* dresid, int* drank, int batch);
int qr_gelsy_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                         int* djpvt, long long stridejpvt, double* dtau, long long stridetau,
                         double* dB, int nrhs, int ldb, long long strideB,
                         double rcond, double* dresid, int* drank, int batch);

/* The pivoted twin of qr_thin_batched: A[:, jpvt] = Q R per matrix, jpvt n ints per matrix (0-based).  Synchronous. */
int qr_thin_pivoted_batched(const double* A, int m, int n, int batch, double* Q, double* R, int* jpvt);

/* Rank-deficient least squares on a packed batch on host pointers (A and B untouched): X n x nrhs per matrix, minimum-norm (minnorm
 * != 0, gelsy) or basic (gelsp); resid (nrhs per matrix), rank (batch ints) and jpvt (n per matrix) may each be NULL.  Creates a plan of
 * its own.  Synchronous.  Returns 0 for any rank. */
int qr_lstsq_pivoted_batched(const double* A, int m, int n, const double* B, int nrhs, int batch, double rcond, int minnorm,
                             double* X, double* resid, int* rank, int* jpvt);

/* ---------------------------------------------------------------------------------------------
 * 8c. Batched singular value decomposition of small matrices: A = U diag(S) V^T for every matrix of a batch (m >= n) -- per-sample PCA,
 * Procrustes / Kabsch alignment, per-element pseudo-inverses, condition numbers, low-rank truncation, what torch.linalg.svd on a batch is
 * used for.  Sections 8 and 8b's conventions hold unchanged: the layout (base + q * stride, column-major, strides in elements), the shape
 * limits (n <= QR_BATCHED_MAX_N, m as qr_batched_max_rows describes), the plan that supplies the stream only, no host wait, QR_E_ARG for
 * bad arguments before anything touches a device, batch == 0 returns 0 after the checks, no atomics, every sum in an order that n alone
 * fixes, results bitwise repeatable and bitwise independent of `batch` and of a matrix's index.
 *
 * Per matrix:
 *   1. A P = Q R by qr_geqp3_batched_dev's kernel.
 *   2. The rank cut: r = the length of the leading run of |R(i,i)| > sqrt(n) * DBL_EPSILON * |R(0,0)| (LAPACK dgejsv's threshold for an
 *      absolute error bound), 0 if R(0,0) == 0.  Rows r..n-1 of R are dropped: the diagonal of a pivoted R bounds every later row, so their
 *      Frobenius norm is at most n eps |R(0,0)|.  The threshold is fixed; there is no rcond argument.
 *   3. One-sided Jacobi on G = (R with rows r.. zeroed)^T, n x n in LDS; its columns r..n-1 are exact zeros and are never touched.  The
 *      pairs come in the round-robin circle ordering of qr_jsvd_round_pairs taken column by column.  For (p, q): a = g_p.g_p, b = g_q.g_q,
 *      c = g_p.g_q; the pair is skipped if a or b is 0, if |c| <= tol sqrt(a) sqrt(b) with tol = sqrt(n) * DBL_EPSILON, or if it is not live
 *      by section 7's rule (a > eps^2 b and b > eps^2 a); otherwise the rotation of the smaller angle, zeta = (b - a) / (2 c),
 *      t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), is applied to G and, when U is wanted, to W (n x n, starts as I).  The iteration ends
 *      with the first sweep that rotated nothing (that sweep is counted), at QR_JSVD_MAX_SWEEPS at the latest.
 *   4. S = the column norms of G, sorted descending and stably; the live columns of V = P times the normalised columns of G.
 *   5. Where r < n, the n - r columns of V that belong to S = 0 complete the live ones to an orthonormal basis (the trailing columns of the
 *      Q of a Householder QR of the live block); the live columns are kept as computed.
 *   6. U = Q [W; 0] by qr_ormqr_batched_dev's kernel: every column of U is a unit vector, and those for S = 0 are Q's columns r..n-1.
 * Pivoting and the rank cut are what make the rank-deficient members of a batch converge (Jacobi on R itself, or on R^T of an unpivoted
 * QR, did not).  Three launches whatever `batch` is (geqp3, Jacobi, ormqr), two when U is not wanted.  n <= 32: one wave per matrix, four
 * matrices per workgroup; above: one workgroup per matrix.
 *
 * Out of scope: a single fused launch; wide matrices (m < n: factor the transpose); n > QR_BATCHED_MAX_N; a caller-chosen threshold.
 * ------------------------------------------------------------------------------------------- */

/* jobu 'U' / 'N' and jobv 'V' / 'N' select the outputs.  dA, djpvt and dtau come back as qr_geqp3_batched_dev leaves them, so
 * qr_ormqr_batched_dev keeps working on them.  dS: n values per matrix, descending and non-negative, exactly 0.0 beyond the rank cut.
 * dU: m x n per matrix (jobu 'N': not referenced, may be NULL); dV: n x n per matrix, V and not V^T (jobv 'N': may be NULL); per matrix
 * A = dU diag(dS) dV^T.  drank (batch ints, may be NULL) = the number of non-zero values; dsweeps (batch ints, may be NULL) = the sweeps
 * used; dinfo (batch ints, required) = 0, or 1 where QR_JSVD_MAX_SWEEPS was reached -- the call still returns 0 and the other matrices
 * are valid.  QR_E_ARG, besides what section 8b rejects: an unknown job letter, dS or dinfo NULL, strideS < n, and for an output that is
 * wanted a NULL pointer, ldu < m, strideU < ldu * n, ldv < n or strideV < ldv * n.  Nothing outside the stated extents is written. */
int qr_gesvd_batched_dev(qr_plan* plan, char jobu, char jobv,
                         double* dA, int m, int n, int lda, long long strideA,
                         int* djpvt, long long stridejpvt, double* dtau, long long stridetau,
                         double* dS, long long strideS,
                         double* dU, int ldu, long long strideU,
                         double* dV, int ldv, long long strideV,
                         int* drank, int* dsweeps, int* dinfo, int batch);

/* The SVD of a packed batch on host pointers (A untouched; lda = m, stride = m * n): S n values per matrix, U m x n, V n x n (column-major,
 * packed) and rank (batch ints); U, V and rank may each be NULL.  Creates a plan of its own.  Synchronous.  Returns QR_E_NOCONV if any
 * matrix reached QR_JSVD_MAX_SWEEPS. */
int qr_svd_batched(const double* A, int m, int n, int batch, double* S, double* U, double* V, int* rank);

/* ---------------------------------------------------------------------------------------------
 * 8d. Batched row append and removal, and sliding-window least squares: sections 6 and 6b for every member of a batch in one launch --
 * recursive least squares per channel, rolling regressions over thousands of series, sliding-window calibration.  Per member the n x n
 * triangle R is stacked on a block of p_add + p_del rows, of which the first p_add are added and the last p_del removed:
 * R'^T R' = R^T R + B^T S B, S = diag(+1 .. +1, -1 .. -1).  Section 8's conventions hold unchanged: the layout (member q at base +
 * q * stride, column-major, strides in elements, packed strides legal, a stride smaller than the block it steps over is QR_E_ARG), the
 * plan that supplies the stream only, no host wait, QR_E_ARG for bad arguments before anything touches a device, batch == 0 returns 0
 * after the checks and launches nothing, no atomics, every sum in an order that (n, nrhs, p_add, p_del) alone fix, results bitwise
 * repeatable and bitwise independent of `batch` and of a member's index.
 *
 * Per column the arithmetic is section 6b's: with sa / sd the sums of squares of the added / removed rows of column j,
 * h = hypot(R(j,j), sqrt(sa)), nd = sqrt(sd), d = (h - nd)(h + nd), beta = -sign(R(j,j)) sqrt(d), tau = (beta - R(j,j)) / beta,
 * v = b / (R(j,j) - beta); a block column that is exactly zero gives tau = 0 and leaves everything untouched; d <= 0 or d not finite is
 * the failure.  The update is unblocked (one reflector at a time, like section 8's factorisation): these calls carry tau, n per member,
 * and no block T.  The strict lower triangle of R is neither read nor written.  Stability is section 6b's.
 *
 * Shapes: 1 <= n, nrhs >= 0, n + nrhs <= QR_BATCHED_MAX_N; p_add >= 0, p_del >= 0, 1 <= p_add + p_del <=
 * qr_tpqrt_batched_max_rows(n + nrhs).  The right-hand sides always ride along as extra columns of the same launch.  One wave per member
 * (four members per workgroup) for n + nrhs <= 32 and p_add + p_del <= 64; otherwise one workgroup per member with both images in LDS.
 *
 * Failure is per member: a member whose removal fails gets its info word and is otherwise not written -- its R, block, tau and
 * right-hand sides are bitwise what they were; the other members are unaffected and the call returns 0.
 * ------------------------------------------------------------------------------------------- */

/* The rows p_add + p_del one call of this section takes beside ncols = n + nrhs columns: 256 for 1 <= ncols <= 32 (one block row per
 * thread of the workgroup), 226 for 33 <= ncols <= 64 (64 columns of the block at a leading dimension of 226 = 2 mod 32 beside the
 * 64 x 65 image of the triangle are 149 568 of the 163 840 bytes of LDS; the next leading dimension, 258, does not fit), 0 otherwise.
 * No device is touched. */
int qr_tpqrt_batched_max_rows(int ncols);

/* [R ; B] -> [R' ; 0] under S for every member: R' over dR's upper triangle (n x n, ldr >= n), V over dB ((p_add + p_del) x n, ldb >=
 * p_add + p_del; reflector j is [e_j ; V(:, j)]), tau (n per member) to dtau.  nrhs > 0: [C1 ; C2] (dC1: n x nrhs, ldc1 >= n; dC2:
 * (p_add + p_del) x nrhs) goes through the same transformation, what qr_tphmqrt_dev computes; nrhs == 0: dC1 and dC2 are not referenced.
 * dinfo (batch device ints): 0, or the failing column + 1; such a member's dR, dB, dtau, dC1 and dC2 are bitwise what they were. */
int qr_tphqrt_batched_dev(qr_plan* plan, double* dR, int n, int ldr, long long strideR,
                          double* dB, int p_add, int p_del, int ldb, long long strideB,
                          double* dtau, long long stridetau,
                          double* dC1, int ldc1, long long strideC1,
                          double* dC2, int ldc2, long long strideC2, int nrhs,
                          int* dinfo, int batch);

/* The p_del == 0 case (LAPACK dtpqrt with L = 0, unblocked, per member): the same kernels, bitwise the same result. */
int qr_tpqrt_batched_dev(qr_plan* plan, double* dR, int n, int ldr, long long strideR,
                         double* dB, int p, int ldb, long long strideB,
                         double* dtau, long long stridetau,
                         double* dC1, int ldc1, long long strideC1,
                         double* dC2, int ldc2, long long strideC2, int nrhs, int batch);

/* Applies the stored reflectors to later right-hand sides [C1 ; C2] (any nrhs >= 1; p_add + p_del <= qr_tpqrt_batched_max_rows(n)):
 * trans 'T' is the transformation that took [R ; B] to [R' ; 0], for any signs; trans 'N' is its inverse and exists for p_del == 0
 * only (QR_E_ARG otherwise).  One launch. */
int qr_tpmqrt_batched_dev(qr_plan* plan, char trans, const double* dV, int p_add, int p_del, int n, int ldv, long long strideV,
                          const double* dtau, long long stridetau,
                          double* dC1, int ldc1, long long strideC1, double* dC2, int ldc2, long long strideC2,
                          int nrhs, int batch);

/* The least-squares accumulator of sections 6 and 6b for a batch: per member R (n x n), Z (n x nrhs), one sum of squares per right-hand
 * side and a row count, all on the device and all zero at the start; nrhs >= 1, n + nrhs <= QR_BATCHED_MAX_N.  The plan must outlive it.
 *   push_dev    folds p >= 1 rows [dA | dB] (dA: p x n, lda >= p; dB: p x nrhs) into every member, in row blocks of at most
 *               qr_tpqrt_batched_max_rows(n + nrhs) rows, one launch each (a push cannot fail, so blocks are committed one by one)
 *   pop_dev     removes p rows that were pushed earlier;  slide_dev adds pnew rows and removes pold rows in one pass, reading the two
 *               pairs of buffers directly.  Both are ONE launch and require p (pnew + pold) <= qr_tpqrt_batched_max_rows(n + nrhs) --
 *               QR_E_ARG above it: the caller feeds blocks.  dinfo (batch device ints): 0; the failing column + 1; or -1 where the
 *               member would be left with fewer than n rows (decided on the device from its row count, before any arithmetic).  On any
 *               non-zero value that member's R, Z, sums and row count are bitwise what they were.
 *   The inputs of all three are untouched.  The sums become max(0, rss + |E_add|^2 - |E_del|^2), E = what the transformation leaves in
 *   the block rows of the right-hand sides.
 *   factor_dev  the device addresses of R, Z (both at a leading dimension of n, packed), the sums (nrhs per member) and the row counts
 *               (any argument may be NULL); valid until destroy, changed by every push / pop / slide
 *   solve_dev   dX (n x nrhs per member, ldx >= n) = R^-1 Z; dresid (nrhs per member, strideresid >= nrhs; may be NULL) = the square
 *               roots of the sums; dinfo: 0, or i + 1 for the smallest i with R(i,i) == 0 (a member that holds fewer than n rows); such
 *               a member's dX holds Z.  Two launches.  The state is untouched.
 *   reset       back to the empty state (stream-ordered);  destroy waits for the plan's stream, then frees.
 * Every call returns 0 without waiting (destroy excepted). */
typedef struct qr_lsacc_batched qr_lsacc_batched;
int qr_lsacc_batched_create(qr_lsacc_batched** acc, qr_plan* plan, int n, int nrhs, int batch);
int qr_lsacc_batched_push_dev(qr_lsacc_batched* acc, const double* dA, int p, int lda, long long strideA,
                              const double* dB, int ldb, long long strideB);
int qr_lsacc_batched_pop_dev(qr_lsacc_batched* acc, const double* dA, int p, int lda, long long strideA,
                             const double* dB, int ldb, long long strideB, int* dinfo);
int qr_lsacc_batched_slide_dev(qr_lsacc_batched* acc, const double* dAnew, int pnew, int ldan, long long strideAn,
                               const double* dBnew, int ldbn, long long strideBn,
                               const double* dAold, int pold, int ldao, long long strideAo,
                               const double* dBold, int ldbo, long long strideBo, int* dinfo);
int qr_lsacc_batched_factor_dev(qr_lsacc_batched* acc, const double** dR, int* ldr, long long* strideR,
                                const double** dZ, int* ldz, long long* strideZ, const double** drss, const int** drows);
int qr_lsacc_batched_solve_dev(qr_lsacc_batched* acc, double* dX, int ldx, long long strideX,
                               double* dresid, long long strideresid, int* dinfo);
int qr_lsacc_batched_reset(qr_lsacc_batched* acc);
int qr_lsacc_batched_destroy(qr_lsacc_batched* acc);

/* Least squares over a moving window for a packed batch of series on host pointers (A: m x n per member, lda = m; B: m x nrhs per
 * member; both untouched).  Window k is rows [k step, k step + window), k = 0 .. (m - window) / step.  X: one n x nrhs solution (ld n)
 * per window per member, member-major (member q's windows one after the other); resid (nrhs per window per member, may be NULL); info:
 * one int per window per member in the same order.  The first window is a push, every later one ONE slide for the whole batch.
 * QR_E_ARG as qr_lstsq_rolling, and for n + nrhs > QR_BATCHED_MAX_N or 2 * step > qr_tpqrt_batched_max_rows(n + nrhs).  Returns
 * QR_E_NOTPD if some slide's info word is non-zero (that member keeps its previous state), else QR_E_SINGULAR if some solve's is; the
 * other entries stay valid.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_rolling_batched(const double* A, int m, int n, const double* B, int nrhs, int batch, int window, int step,
                             double* X, double* resid, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8e. Batched minimum-norm solutions: transposed and wide systems.  Section 5 for every member of a batch -- underdetermined fits,
 * redundant-manipulator inverse kinematics (a 6 x 7 Jacobian per sample), constraint projection per element, minimum-norm
 * interpolation weights; what torch.linalg.lstsq on a batch of wide matrices is used for.  With F = Q R (rows x cols, rows >= cols,
 * full rank) the minimum-norm solution of F^T X = B is X = Q [R^-T B ; 0]; a wide system A X = B is the same thing with F = A^T.
 * Throughout, (rows, cols) is the shape of the tall matrix that is factored: (m, n) for gels_t and minnorm, (n, m) for gels_wide.
 *
 * Section 8's conventions hold unchanged: member q at base + q * stride, column-major, strides in elements; the plan supplies the
 * stream only; no call waits on the host; bad arguments return QR_E_ARG before anything touches a device (what section 8 rejects, and
 * besides: m < n or m > n where the call wants the other, ldb below the taller of B and X, ldf < n, strideF < ldf * m, dinfo, dF or
 * dtau NULL); batch == 0 returns 0 after the checks and launches nothing; no atomics, every sum in an order that (rows, cols, nrhs)
 * alone fix; results bitwise repeatable and bitwise independent of `batch` and of a member's index; the route follows from the shape
 * alone.
 *
 * Routes.  The fused calls hold the right-hand sides beside the matrix as nrhs more columns of height rows: one wave per member (four
 * members per workgroup) for rows <= 64 and cols + nrhs <= 32, otherwise one workgroup per member with [F | X] in LDS.  The
 * factorisation step is section 8's, the same code, and does not touch the right-hand sides: dA / dtau of
 * qr_gels_t_batched_dev and dF / dtau of qr_gels_wide_batched_dev are bitwise those of qr_geqrf_batched_dev (on the same matrix, on the
 * explicit transpose) whenever (rows, cols) and (rows, cols + nrhs) take the same route, and always on the composed routes.  Then
 * R^T y = b by forward substitution, y_k = (b_k - sum_{l<k} R(l,k) y_l) / R(k,k) with l ascending, and X = H_0 .. H_{cols-1} [y ; 0]
 * with the reflectors applied cols-1 down to 0, rows >= cols starting at exact zero and tau == 0 reflectors skipped (a square
 * member's last column, and a 1 x 1, stay exact).
 *
 * The info word: dinfo[q] is 0, or i + 1 for the smallest i with R(i,i) == 0 exactly (a zero row of a wide A, a zero column of F).
 * Such a member is all or nothing, as in section 8d: its dB is bitwise what it was on entry, every row included; its factors are
 * still written by the factoring calls; the other members are unaffected and the call returns 0.  Dependence to rounding is NOT
 * detected: as for qr_gels_batched_dev, a member that is rank-deficient only to rounding gets a huge X and info == 0.
 *
 * Out of scope: rank-deficient wide systems (they need a pivoted wide factorisation and a complete orthogonal decomposition for
 * m < n); blocked / MFMA variants; the entry points of sections 8 to 8d are unchanged and keep answering QR_E_ARG for m < n.
 * ------------------------------------------------------------------------------------------- */

/* The solve from factors that exist (m >= n), in the layout of qr_geqrf_batched_dev or qr_geqp3_batched_dev (for pivoted factors the
 * system solved is (A P)^T X = B): factor once, solve many.  dB is m x nrhs per member, ldb >= m, any nrhs >= 1: rows 0..n-1 hold B on
 * entry, rows n..m-1 are ignored; on return dB = X = Q [R^-T B ; 0].  One launch for any nrhs. */
int qr_minnorm_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA,
                           const double* dtau, long long stridetau,
                           double* dB, int nrhs, int ldb, long long strideB, int* dinfo, int batch);

/* LAPACK dgels ('T', m >= n) per member: dA is factored in place (R, V, dtau as qr_geqrf_batched_dev leaves them), then the above.  One
 * fused launch when n + nrhs <= QR_BATCHED_MAX_N and m <= qr_batched_max_rows(n + nrhs) (or m x (n + nrhs) passes section 8's
 * narrower-fit rule); otherwise qr_geqrf_batched_dev followed by qr_minnorm_batched_dev: two launches. */
int qr_gels_t_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                          double* dtau, long long stridetau,
                          double* dB, int nrhs, int ldb, long long strideB, int* dinfo, int batch);

/* dD_q (cols x rows, ldd >= cols) = dS_q^T (dS_q: rows x cols, lds >= rows) for every member, out of place; nothing outside the
 * cols x rows block is written.  Any shape with rows, cols <= 512.  Reads and writes both run along contiguous addresses, through LDS.
 * It serves the composed wide route, and lets a caller reach dgels 'T' of a wide matrix as transpose plus qr_gels_batched_dev. */
int qr_transpose_batched_dev(qr_plan* plan, const double* dS, int rows, int cols, int lds, long long strideS,
                             double* dD, int ldd, long long strideD, int batch);

/* LAPACK dgels ('N', m <= n) per member: the minimum-norm solution of A X = B.  m <= QR_BATCHED_MAX_N, and n x m must fit as section 8
 * describes: n <= qr_batched_max_rows(m), or m < 64 and n rows of m columns pass the narrower-fit rule (64 x 256 and 40 x 300 are
 * taken, 64 x 257 and 64 x 300 are not).  dA (m x n, lda >= m) is not modified.  dF (n x m, ldf >= n, strideF >= ldf * m) and dtau
 * (m per member) receive the factors of A^T in qr_geqrf_batched_dev's layout: qr_minnorm_batched_dev(plan, dF, n, m, ...) solves
 * again.  dB is n x nrhs, ldb >= n: rows 0..m-1 hold B on entry; on return it holds X.  One fused launch when
 * m + nrhs <= QR_BATCHED_MAX_N and n x (m + nrhs) fits: the kernel reads A through the transposed index map straight into registers /
 * LDS.  Otherwise transpose, geqrf, minnorm: three launches. */
int qr_gels_wide_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA,
                             double* dF, int ldf, long long strideF, double* dtau, long long stridetau,
                             double* dB, int nrhs, int ldb, long long strideB, int* dinfo, int batch);

/* The wide call on a packed batch on host pointers (A: m x n, B: m x nrhs per member, m <= n, both untouched): X n x nrhs per member,
 * info[batch] as dinfo above.  Returns QR_E_SINGULAR if any info entry is non-zero (X of such a member holds no solution; the others
 * are valid); QR_E_ARG for m > n.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_minnorm_batched(const double* A, int m, int n, const double* B, int nrhs, int batch,
                             double* X, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8f. Batched damped least squares: ridge regression and the Levenberg-Marquardt step.  Per member and per lambda_k of a list of nlam,
 * min |A x - b|^2 + lambda_k^2 |D x|^2 with D = diag(d) -- damped inverse kinematics, the inner step of per-pixel curve fitting, a ridge
 * regression tuned over a grid of lambda.  A is factored once; every lambda then costs O(n^3): the n rows of S = lambda D are
 * eliminated against the n x n triangle R by Householder reflectors with Z = the top of Q^T b riding along (MINPACK qrsolv; LAPACK
 * dtpqrt with L = n, a triangle stacked on a triangle), and R~ x = z~ is solved.
 *
 * Section 8's conventions hold unchanged: member q at base + q * stride, column-major, strides in elements; the plan supplies the
 * stream only; no call waits on the host; bad arguments return QR_E_ARG before anything touches a device; batch == 0 returns 0 after the
 * checks and launches nothing; no atomics; every sum in an order that the shape arguments alone fix; results bitwise repeatable and
 * bitwise independent of `batch`, of a member's index, of nlam and of a lambda's position in its list (every lambda starts from the
 * untouched factors).  One exception to the stride rule: strideD == 0 and stridelam == 0 are legal and mean one d / one list of lambda
 * shared by every member; any other value must be at least n / nlam.
 *
 * The operands.  dD: n doubles per member, NULL means d = 1.  dlam: nlam >= 1 doubles per member.  Only (lambda d_i)^2 matters to the
 * mathematics; the signs are the caller's; non-finite values are not detected.
 *
 * The step.  With [R | Z] (n x (n + nrhs)) and the block [S | 0], for j = 0 .. n-1, x = S(0..j, j) (row i of the block has its
 * non-zeros in columns >= i), ssq = |x|^2: ssq == 0 exactly gives tau = 0 and touches nothing; otherwise beta, tau and v are section
 * 8's dlarfg values of (R(j,j), x), and columns j+1 .. n+nrhs-1 take the reflector [e_j ; v].  R~ overwrites a working copy: the
 * caller's R and Z are read only.  Then x_k = R~^-1 z~ by the back substitution of section 8.
 *
 * Per (member, lambda_k) the calls write: the solution (n x nrhs) into columns k * nrhs .. (k + 1) * nrhs - 1 of dX (ldx >= n, strideX
 * >= ldx * nlam * nrhs); dxnorm = |D x|_2 and dresid = |A x - b|_2 (nlam * nrhs doubles per member each, packed, in the same order;
 * either may be NULL), the latter as sqrt(|R x - z|^2 + rss) with R x - z formed from the untouched R and Z and rss the tail sum of
 * squares of Q^T b; dinfo (nlam ints per member, packed): 0, or i + 1 for the smallest i with R~(i,i) == 0 exactly (lambda = 0 on a
 * singular R, d_i = 0 on a zero column).  The X, xnorm and resid entries of a failing pair are not written at all; every other pair is
 * unaffected and the call returns 0.
 *
 * Routes.  n + nrhs <= 32: one wave per member, four members per workgroup, lane i holding row i of the factors, of the working copy
 * and of the block in registers.  Otherwise (n + nrhs <= QR_BATCHED_MAX_N): one workgroup per member with the three images in LDS.
 *
 * Out of scope: a general D for wide members; a fused launch on the workgroup route; generalised cross-validation; blocked / MFMA
 * variants.  (The trust-region search for lambda is section 8g.)
 * ------------------------------------------------------------------------------------------- */

/* The damped solves from factors that exist, one launch.  dR: n x n, ldr >= n, only the upper triangle is read; dZ: n x nrhs, ldz >= n,
 * the top of Q^T B; drss (may be NULL: 0): nrhs doubles per member, packed, the tail sums of squares.  1 <= n, nrhs >= 1,
 * n + nrhs <= QR_BATCHED_MAX_N.  djpvt (may be NULL; n ints per member, stridejpvt >= n) passes the factors of qr_geqp3_batched_dev for
 * A P = Q R: S uses d[jpvt[j]] in column j and the solution is scattered back so that X is in the caller's column order (what MINPACK
 * lmpar / qrsolv do); an entry outside [0, n) is read as the identity.  flip != 0 reads the triangle as U(i, k) = R(n-1-k, n-1-i) with
 * Z and the rows of the solution reversed -- the transpose of R made upper triangular, the wide case below; dD and djpvt must then be
 * NULL. */
int qr_damped_batched_dev(qr_plan* plan, const double* dR, int n, int ldr, long long strideR,
                          const double* dZ, int nrhs, int ldz, long long strideZ, const double* drss,
                          const int* djpvt, long long stridejpvt, const double* dD, long long strideD,
                          const double* dlam, int nlam, long long stridelam, int flip,
                          double* dX, int ldx, long long strideX, double* dxnorm, double* dresid, int* dinfo, int batch);

/* m >= n: factor and solve.  dA and dtau come back bitwise as qr_geqrf_batched_dev leaves them; dB (m x nrhs, ldb >= m) comes back as
 * Q^T B in all rows -- not overwritten by a solution, so qr_damped_batched_dev can damp again later from dA and dB; rss is taken from
 * rows n .. m-1.  The shape limits are qr_gels_batched_dev's, and n + nrhs <= QR_BATCHED_MAX_N.  ONE launch for m <= 64 and
 * n + nrhs <= 32 (section 8's wave factorisation of [A | B], then the lambda loop on the registers the factors are in; at lambda = 0
 * X is bitwise qr_gels_batched_dev's); otherwise qr_geqrf_batched_dev, qr_ormqr_batched_dev 'T' and qr_damped_batched_dev: three. */
int qr_gels_damped_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                               double* dtau, long long stridetau,
                               double* dB, int nrhs, int ldb, long long strideB,
                               const double* dD, long long strideD, const double* dlam, int nlam, long long stridelam,
                               double* dX, int ldx, long long strideX, double* dxnorm, double* dresid, int* dinfo, int batch);

/* m < n with D = I (damped inverse kinematics): x = Q [y ; 0] with A^T = Q R and y the minimiser of |R^T y - b|^2 + lambda^2 |y|^2,
 * which is qr_damped_batched_dev with flip on R.  dA (m x n, lda >= m) is not modified; dF (n x m, ldf >= n) and dtau (m per member)
 * receive the factors of A^T as in qr_gels_wide_batched_dev; dB (m x nrhs, ldb >= m) is read only; dX is n x (nlam * nrhs), ldx >= n;
 * dxnorm = |x|, dresid = |A x - b|.  The limits are qr_gels_wide_batched_dev's with m < n, and m + nrhs <= QR_BATCHED_MAX_N.  Four
 * launches: transpose, geqrf, the damped solves writing [y ; 0], one ormqr 'N' over all nlam * nrhs columns -- which also runs over the
 * columns of a failing pair: those hold no solution. */
int qr_gels_damped_wide_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA,
                                    double* dF, int ldf, long long strideF, double* dtau, long long stridetau,
                                    const double* dB, int nrhs, int ldb, long long strideB,
                                    const double* dlam, int nlam, long long stridelam,
                                    double* dX, int ldx, long long strideX, double* dxnorm, double* dresid, int* dinfo, int batch);

/* qr_damped_batched_dev on the state of a batched accumulator (section 8d): its R, Z and sums, one launch, the state untouched.  A
 * member that holds fewer than n rows, or none, is solvable for lambda > 0 and gets info 0. */
int qr_lsacc_batched_solve_damped_dev(qr_lsacc_batched* acc, const double* dD, long long strideD,
                                      const double* dlam, int nlam, long long stridelam,
                                      double* dX, int ldx, long long strideX, double* dxnorm, double* dresid, int* dinfo);

/* The damped solves of a packed batch on host pointers (A: m x n, B: m x nrhs per member, both untouched; D: n per member or NULL; lam:
 * nlam per member): X n x (nlam * nrhs) per member, xnorm and resid (nlam * nrhs per member; may be NULL), info (nlam per member).
 * m >= n goes the tall route, m < n the wide route, which requires D == NULL.  Returns QR_E_SINGULAR if any info entry is non-zero.
 * Creates a plan of its own.  Synchronous. */
int qr_lstsq_damped_batched(const double* A, int m, int n, const double* B, int nrhs, int batch,
                            const double* D, const double* lam, int nlam,
                            double* X, double* xnorm, double* resid, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8g. Batched trust-region step: the lambda of section 8f found on the device.  Per member, given a radius Delta > 0, the calls find
 * lambda >= 0 and x = argmin |A x - b|^2 + lambda^2 |D x|^2 such that either lambda = 0 and |D x| <= (1 + rtol) Delta, or
 * | |D x| - Delta | <= rtol Delta -- the inner step of a batched Levenberg-Marquardt solver (per-pixel curve fitting, damped inverse
 * kinematics with a step limit), whose callers hold a radius per member, not a lambda.  One right-hand side per member: several would
 * each need a lambda of their own.  The whole search of every member runs inside one launch; members take different numbers of
 * iterations side by side and nothing waits on the host.
 *
 * The method is MINPACK lmpar (More 1978) with MINPACK's par = lambda^2; it iterates on par, and reports and eliminates with
 * lambda = sqrt(par).
 *   1. Gauss-Newton step.  nsing = the first i with R(i,i) == 0 exactly, or n.  x solves the leading nsing x nsing system, the rest of x
 *      is 0.  fp = |D x| - Delta.  fp <= rtol Delta: lambda = 0, iter = 0, status 1, done.
 *   2. Bounds.  parl = fp / (Delta |w|^2) with R^T w = D^2 x / |D x| (in pivoted order) if nsing == n, else 0.  paru = |g| / Delta with
 *      g_j = (sum over i <= j of R(i,j) z_i) / d[jpvt[j]] (a column with d == 0 contributes nothing); if that is 0, paru = DBL_MIN /
 *      min(Delta, 0.1).
 *   3. Start.  par = min(max(lambda0^2, parl), paru); if par == 0, par = |g| / |D x|.
 *   4. At most maxit iterations: if par == 0, par = max(DBL_MIN, 0.001 paru); lambda = sqrt(par); section 8f's elimination of
 *      lambda D against the untouched factors, the same arithmetic in the same order; R~ x = z~; fp = |D x| - Delta.  Leave with status 0
 *      if |fp| <= rtol Delta; with status 2 if parl == 0 and fp <= the previous fp < 0; with status 3 if the count is reached.  Otherwise
 *      R~^T w = D^2 x / |D x|, parc = fp / (Delta |w|^2); fp > 0 raises parl to par, fp < 0 lowers paru to par; par = max(parl, par + parc).
 * MINPACK's constants are rtol = 0.1 and maxit = 10; here 0 < rtol < 1 and maxit >= 1 are arguments.
 *
 * Range.  The search is good for factors, right-hand sides and radii whose entries, together with the products of one entry of R and
 * one of z, lie inside 2^+-1000 (about 1e+-301): |g| is formed as MINPACK's enorm forms it, with the entries scaled by a power of two
 * where their squares would leave the double range (the plain sum, bit for bit, while the largest |g_j| lies inside 2^+-256), so that
 * g -- a product of two data quantities -- may be as large or small as its own value allows.  |D x| and |w| are plain sums of squares of
 * quantities of the data's own size: good inside 1e+-150, the range of the library's other norms.
 *
 * Section 8's conventions hold as in 8f, and jpvt, dD, flip, drss and the stride rules are exactly qr_damped_batched_dev's.  ddelta and
 * dlam0 (the starting guess for lambda; may be NULL: 0) hold one double per member; a stride of 0 means shared, any other must be >= 1.
 *
 * Per member the calls write: dX (n rows, one column, ldx >= n, strideX >= ldx), dlam (the lambda found), dxnorm = |D x|, dresid (as in
 * 8f: sqrt(|R x - z|^2 + rss) from the untouched factors), diter (the number of eliminations), dstatus (0 converged; 1 the Gauss-Newton
 * step accepted, lambda = 0; 2 left by the lower-bound clause, MINPACK's exit on a singular R; 3 maxit reached) and dinfo: 0; i + 1 for
 * an exactly zero R~(i,i) in an elimination, as in 8f; -1 for a member whose Delta is not a finite positive number.  One entry per
 * member each, packed; dxnorm, dresid, diter and dstatus may be NULL.  A member with info != 0 has nothing else written; its neighbours
 * are unaffected and the call returns 0.  Because the elimination runs on the stored, rounded lambda = sqrt(par), the X, xnorm and resid
 * of a member are bitwise what qr_damped_batched_dev returns for the lambda in dlam.
 *
 * Routes.  n + 1 <= 32: one wave per member, four members per workgroup, the layout of 8f's wave route; every loop decision is taken on
 * a value that a wave butterfly left identical in all lanes.  Otherwise (n <= QR_BATCHED_MAX_N - 1): one workgroup per member with 8f's
 * three LDS images, thread 0 publishing every decision in an LDS word that all threads read after a barrier.  Both compile to no
 * scratch memory.
 *
 * The outer Levenberg-Marquardt loop (the gain ratio, the update of Delta) is section 8m, which runs this search's device code.
 *
 * Out of scope: several right-hand sides per
 * member; a general D for wide members; a fused launch on the workgroup route; blocked / MFMA variants of the elimination.
 * ------------------------------------------------------------------------------------------- */

/* The step from factors that exist, one launch.  dR: n x n, ldr >= n, only the upper triangle is read; dZ: n rows, ldz >= n, strideZ >=
 * ldz, the top of Q^T b; drss (may be NULL: 0): one double per member.  1 <= n <= QR_BATCHED_MAX_N - 1. */
int qr_trust_batched_dev(qr_plan* plan, const double* dR, int n, int ldr, long long strideR,
                         const double* dZ, int ldz, long long strideZ, const double* drss,
                         const int* djpvt, long long stridejpvt, const double* dD, long long strideD,
                         const double* ddelta, long long stridedelta, const double* dlam0, long long stridelam0,
                         double rtol, int maxit, int flip,
                         double* dX, int ldx, long long strideX, double* dlam, double* dxnorm, double* dresid,
                         int* diter, int* dstatus, int* dinfo, int batch);

/* m >= n: factor and search.  dA, dtau and dB (m rows, ldb >= m; Q^T b in all rows on return) come back as
 * qr_gels_damped_batched_dev leaves them; the shape limits are its own with nrhs = 1.  ONE launch for m <= 64 and n + 1 <= 32 (section
 * 8's wave factorisation of [A | b], then the same search on the registers the factors are in; where the Gauss-Newton step is accepted
 * X is bitwise qr_gels_batched_dev's); otherwise qr_geqrf_batched_dev, qr_ormqr_batched_dev 'T' and qr_trust_batched_dev: three. */
int qr_gels_trust_batched_dev(qr_plan* plan, double* dA, int m, int n, int lda, long long strideA,
                              double* dtau, long long stridetau, double* dB, int ldb, long long strideB,
                              const double* dD, long long strideD,
                              const double* ddelta, long long stridedelta, const double* dlam0, long long stridelam0,
                              double rtol, int maxit,
                              double* dX, int ldx, long long strideX, double* dlam, double* dxnorm, double* dresid,
                              int* diter, int* dstatus, int* dinfo, int batch);

/* m < n with D = I: a minimum-norm step of bounded length (inverse kinematics with a step limit).  x = Q [y ; 0] with A^T = Q R and
 * |x| = |y|, so the radius applies to y.  The operands and limits are qr_gels_damped_wide_batched_dev's with nrhs = 1 (m <=
 * QR_BATCHED_MAX_N - 1); dX has n rows, ldx >= n.  Four launches: transpose, geqrf, the search with flip writing [y ; 0], one ormqr 'N'
 * -- which also runs over the column of a member with an info word: that holds no solution. */
int qr_gels_trust_wide_batched_dev(qr_plan* plan, const double* dA, int m, int n, int lda, long long strideA,
                                   double* dF, int ldf, long long strideF, double* dtau, long long stridetau,
                                   const double* dB, int ldb, long long strideB,
                                   const double* ddelta, long long stridedelta, const double* dlam0, long long stridelam0,
                                   double rtol, int maxit,
                                   double* dX, int ldx, long long strideX, double* dlam, double* dxnorm, double* dresid,
                                   int* diter, int* dstatus, int* dinfo, int batch);

/* qr_trust_batched_dev on the state of a batched accumulator (section 8d) with nrhs == 1: its R, Z and sums, one launch, the state
 * untouched. */
int qr_lsacc_batched_solve_trust_dev(qr_lsacc_batched* acc, const double* dD, long long strideD,
                                     const double* ddelta, long long stridedelta, const double* dlam0, long long stridelam0,
                                     double rtol, int maxit,
                                     double* dX, int ldx, long long strideX, double* dlam, double* dxnorm, double* dresid,
                                     int* diter, int* dstatus, int* dinfo);

/* The step of a packed batch on host pointers (A: m x n, b: m per member, both untouched; D: n per member or NULL; delta: one per member;
 * lam0: one per member or NULL): X n per member, lam, and xnorm, resid, iter, status (any may be NULL), info, one per member.  m >= n
 * goes the tall route, m < n the wide route, which requires D == NULL.  iter and status of a member with an info word read 0.  Returns
 * QR_E_SINGULAR if any info entry is non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_trust_batched(const double* A, int m, int n, const double* b, int batch,
                           const double* D, const double* delta, const double* lam0, double rtol, int maxit,
                           double* X, double* lam, double* xnorm, double* resid, int* iter, int* status, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8h. Batched equality-constrained least squares: LAPACK dgglse's problem for every member of a batch,
 *
 *         min |A x - b|_2  subject to  C x = d,      A: m x n, C: p x n, 1 <= p <= n, m >= 1, m + p >= n,
 *
 * for nrhs >= 1 pairs (b, d), n + nrhs <= QR_BATCHED_MAX_N -- inverse kinematics with a contact constraint that must hold exactly, fits
 * that interpolate given points or conserve a sum, the equality-constrained Gauss-Newton step inside the loops of 8f and 8g.  One launch
 * whatever the batch size; nothing waits on the host.
 *
 * The method is the null-space method (Bjorck, Numerical Methods for Least Squares Problems, 5.1; Lawson & Hanson ch. 20):
 *   1. C^T = Q_c [R_c ; 0] by Householder QR (section 8's column step on C read through the transposed index map).
 *   2. R_c^T y1 = d.
 *   3. A~ = A Q_c: every row of A takes the p reflectors from the right.
 *   4. r = b - A~(:, 0:p) y1.
 *   5. Householder QR of A~(:, p:n) with r and A~(:, 0:p) riding along; R_a y2 = (Q_a^T r)(0 : n-p).
 *   6. x = Q_c [y1 ; y2].
 *   7. resid = |(Q_a^T r)(n-p : m)|_2 = |A x - b|.
 *   8. The Lagrange multipliers lambda of A^T (A x - b) + C^T lambda = 0: R_c lambda = g with
 *      g_i = sum over rows >= n-p of (Q_a^T A~(:, 0:p))(row, i) (Q_a^T r)(row).
 * p == n: x is fixed by the constraints, A only feeds resid and lambda.  m == n - p: resid is an exact 0.
 *
 * Section 8's conventions hold: member q lives at base + q * stride, column-major, strides count doubles; the plan supplies the stream
 * only; batch == 0 returns 0 after the argument checks and launches nothing.  The four inputs are never written.
 *
 * dinfo[q]: 0; i + 1 for the smallest i < p with R_c(i,i) == 0 exactly (a zero row of C produces this); p + i + 1 for the smallest i with
 * R_a(i,i) == 0 exactly.  Such a member is all or nothing: its X, L and resid are not written at all; the other members are unaffected
 * and the call returns 0.  Dependence to rounding among the rows of C, or among the columns of A restricted to the null space of C, is
 * NOT detected, as in sections 8 and 8e: the result is then as large and as wrong as the conditioning makes it.
 *
 * Routes, chosen from the shape alone.  m <= 64 and n + nrhs <= 32: one wave per member, four members per workgroup.  Otherwise one
 * workgroup per member with [A~ | rhs] and the factors of C^T in LDS, for m <= qr_gglse_batched_max_rows(n, p, nrhs).  A member's results
 * do not depend on the batch size or on its place in the batch, and repeated calls are bitwise equal.
 *
 * Out of scope: solving again from stored factors (the call returns none); p == 0 (qr_gels_batched_dev); rank-deficient C or [A ; C];
 * inequality constraints; n + nrhs > QR_BATCHED_MAX_N; shapes that do not fit LDS; a single-matrix variant.
 * ------------------------------------------------------------------------------------------- */

/* the largest m taken for (n, p, nrhs) (at most 512); 0 if (n, p, nrhs) is not taken at all.  No device is touched. */
int qr_gglse_batched_max_rows(int n, int p, int nrhs);

/* dA: m x n (lda >= m, strideA >= lda * n); dC: p x n (ldc >= p, strideC >= ldc * n); dB: m x nrhs (ldb >= m, strideB >= ldb * nrhs);
 * dD: p x nrhs (ldd >= p, strideD >= ldd * nrhs); dX: n x nrhs (ldx >= n, strideX >= ldx * nrhs); dL (may be NULL): the multipliers,
 * p x nrhs (ldl >= p, strideL >= ldl * nrhs); dresid (may be NULL): nrhs per member, strideres >= nrhs apart; dinfo: one per member.
 * QR_E_ARG, before any device is touched, for a shape or an operand outside these rules. */
int qr_gglse_batched_dev(qr_plan* plan,
                         const double* dA, int m, int n, int lda, long long strideA,
                         const double* dC, int p, int ldc, long long strideC,
                         const double* dB, int ldb, long long strideB,
                         const double* dD, int ldd, long long strideD,
                         int nrhs,
                         double* dX, int ldx, long long strideX,
                         double* dL, int ldl, long long strideL,
                         double* dresid, long long strideres,
                         int* dinfo, int batch);

/* The same for a packed batch on host pointers (A: m x n, C: p x n, b: m x nrhs, d: p x nrhs per member, all untouched): X n x nrhs, L
 * p x nrhs and resid nrhs per member (L and resid may be NULL), info one per member; X, L and resid of a member with an info word read 0.
 * Returns QR_E_SINGULAR if any info word is non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_constrained_batched(const double* A, int m, int n, const double* C, int p,
                                 const double* b, const double* d, int nrhs, int batch,
                                 double* X, double* L, double* resid, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8i. Batched bound-constrained least squares: for every member of a batch
 *
 *         min |A x - b|_2  subject to  lo <= x <= hi,      A: m x n, m >= n, 1 <= n <= QR_BATCHED_MAX_N - 1, one b per member,
 *
 * each lo_j may be -inf and each hi_j +inf -- actuator and joint limits in the fits and control steps of 8 to 8h, non-negative
 * abundances or concentrations (NNLS: lo = 0, hi = +inf), the box-constrained Gauss-Newton or Levenberg-Marquardt step.  Clipping an
 * unconstrained solution is the wrong answer; an active-set loop on the host costs a launch, a copy and a host wait per change of the
 * set.  Here the active-set loop of every member runs on the device: one launch whatever the batch size; nothing waits on the host.
 *
 * The method is bounded-variable least squares (Lawson & Hanson, Solving Least Squares Problems, ch. 23; Stark & Parker, BVLS).  The
 * bound set holds the variables at a bound (state -1 at lo, +1 at hi), the free set F the rest (state 0).  Per member:
 *   1. Start.  A variable with a finite lo starts at lo, otherwise at a finite hi; one with both bounds infinite is free from the start
 *      and can never be bound.  x holds those bounds, 0 for the free ones.  The elimination count it = 0, no variable is banned.
 *   2. Outer test (skipped on the first pass if a variable is free).  w = A^T (b - A x) from the untouched A.  Among the bound,
 *      non-banned variables with lo_j < hi_j the largest of w_j (at lo) and -w_j (at hi), ties to the smallest index.  None > 0: done,
 *      info 0.  Otherwise that variable t is freed.
 *   3. Elimination.  it == maxit: done, info n + 1.  Otherwise ++it; r = b - A_B x_B; Householder QR of A(:, F), columns in increasing
 *      index order, with r riding along; R z = (Q^T r)(0 : |F|).  An exactly zero R(i,i): info j + 1, j that column's index in A.
 *   4. Anti-cycling, on the first elimination after t was freed: z_t on or outside the bound t left puts t back and bans it; go to 2.
 *   5. Accept.  lo_F <= z <= hi_F: x_F = z, the bans are lifted, go to 2.
 *   6. Blocked step.  alpha_j = (bound_j - x_j) / (z_j - x_j) over the free j with z_j outside a bound; the smallest, ties to the
 *      smallest index k; x_F += alpha (z - x_F); x_k is set to its bound exactly and bound, and so is every other free variable that
 *      now lies on or outside a bound.  Go to 3.
 * Every candidate is factored from scratch from the untouched A.  it counts every elimination and it <= maxit is the only loop bound;
 * maxit <= 0 means 3 n.  A comparison with a NaN is false and leads towards the count: no input makes a loop run longer.
 *
 * Section 8's conventions hold: member q lives at base + q * stride, column-major, strides count elements; the plan supplies the stream
 * only; batch == 0 returns 0 after the argument checks and launches nothing.  A and b are never written.
 *
 * Outputs, with lo <= x <= hi holding exactly: x; state (-1 / 0 / +1 per variable); w = A^T (b - A x) recomputed from the untouched A at
 * the returned x (w_j <= 0 at lo and >= 0 at hi up to rounding where info is 0, about 0 on the free ones); resid = |A x - b| formed
 * from A and the returned x; iter, the elimination count.
 *
 * dinfo[q]: 0; -1 for bounds that are no box (lo_j > hi_j, a NaN bound, lo_j == +inf or hi_j == -inf) and j + 1 for an exactly zero
 * R(i,i) on free column j: nothing but info is written for such a member; n + 1 at maxit eliminations: the outputs ARE written, the
 * last iterate (feasible), its state, its w and resid -- a caller with a real-time budget takes it.  lo_j == hi_j is legal: state -1,
 * never freed.  The other members are unaffected and the call returns 0.  Dependence to rounding among free columns is NOT detected.
 *
 * Routes, chosen from the shape alone.  m <= 64 and n + 1 <= 32: one wave per member, four members per workgroup.  Otherwise one
 * workgroup per member with the image [A_F | r] in LDS, for m <= qr_bvls_batched_max_rows(n): the largest m <= 512 with
 * 8 ((n + 1) ld(m) + 6 n + 72) bytes within 160 KiB, ld(m) the smallest value >= m that is 2 mod 32.  A member's results do not depend
 * on the batch size or on its place in the batch, and repeated calls are bitwise equal.
 *
 * Out of scope: several right-hand sides per member; m < n; general linear inequalities, or bounds combined with 8h's equalities; a warm
 * start from a given state; QR updating across changes of the free set; rank deficiency to rounding; a single-matrix variant; blocked
 * or MFMA variants.
 * ------------------------------------------------------------------------------------------- */

/* the largest m taken for n unknowns (at most 512); 0 if n is not taken (n < 1 or n > QR_BATCHED_MAX_N - 1).  No device is touched. */
int qr_bvls_batched_max_rows(int n);

/* dA: m x n (lda >= m, strideA >= lda * n); dB: m per member (strideB >= m); dlo, dhi: n per member, stridebnd apart (0: one vector
 * shared by all members, else >= n), either may be NULL: that side is unbounded; dX: n per member (strideX >= n); dW (may be NULL): n
 * per member (strideW >= n); dstate (may be NULL): n ints per member (stridestate >= n); dresid, diter (may be NULL) and dinfo: one per
 * member.  QR_E_ARG, before any device is touched, for a shape or an operand outside these rules (stridebnd is checked even when both
 * bound pointers are NULL). */
int qr_bvls_batched_dev(qr_plan* plan,
                        const double* dA, int m, int n, int lda, long long strideA,
                        const double* dB, long long strideB,
                        const double* dlo, const double* dhi, long long stridebnd,
                        int maxit,
                        double* dX, long long strideX,
                        double* dW, long long strideW,
                        int* dstate, long long stridestate,
                        double* dresid, int* diter,
                        int* dinfo, int batch);

/* The same for a packed batch on host pointers (A: m x n, b: m, lo and hi: n per member, either may be NULL, all untouched): X n, W n
 * and state n per member, resid, iter and info one per member (W, state, resid and iter may be NULL); the outputs of a member with info
 * -1 or j + 1 read 0.  Returns QR_E_SINGULAR if any info word is non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_bounded_batched(const double* A, int m, int n, const double* b, const double* lo, const double* hi,
                             int maxit, int batch, double* X, double* W, int* state, double* resid, int* iter, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8j. Batched robust and weighted least squares: for every member of a batch
 *
 *         min  sum_i p_i rho((b - A x)_i / s),      A: m x n, m >= n, 1 <= n <= QR_BATCHED_MAX_N - 1, one b per member,
 *
 * with prior weights p_i >= 0 per observation (an inverse variance; p_i = 0 masks a missing sample or a saturated pixel without a
 * different m per member) and rho the squared, the Huber or the Tukey bisquare loss -- the per-pixel fits, rolling regressions and
 * calibrations of 8 to 8i when one bad sample must not move the answer.  The method is iteratively reweighted least squares with a MAD
 * scale (Holland & Welsch 1977; MASS::rlm, statsmodels.RLM).  A host loop costs, per reweighting, a scaled copy of the batch, a
 * launch, a residual pass, a median, a weight pass and a host wait, and runs as many rounds as the slowest member needs.  Here the loop of
 * every member runs on the device: one launch whatever the batch size; nothing waits on the host.
 *
 * Per member:
 *   1. Checks.  A p_i that is negative, NaN or inf, or a given scale that is not a finite positive number: info -1.  Rows with
 *      p_i == 0 are excluded: they are read as exact zeros whatever they hold, so a NaN in such a row of A or b is harmless.
 *   2. Start.  The robust weights w_i = 1, the solve count it = 0.  With dX0 (and a robust loss) x = X0 and step 4 comes first: a
 *      bisquare fit started from a Huber fit.  Otherwise step 3.
 *   3. Solve.  c_i = p_i w_i.  Fewer than n rows with c_i > 0: info -2.  it == maxit: status 3, done.  Otherwise ++it; row i of [A | b]
 *      from the untouched inputs times sqrt(c_i); Householder QR with b riding along; R x = (Q^T b)(0 : n).  An exactly zero R(i,i):
 *      info i + 1.
 *   4. Residual, scale, weights.  r = b - A x from the untouched A.  QR_LOSS_LS: status 0, done.  s = the given scale, or
 *      median{|r_i| : p_i > 0} / 0.6744897501960817 (an even count: half the sum of the two middle values).  s == 0 (more than half the
 *      rows fitted exactly): status 2, w = 1, done.  u_i = |r_i| / s.  Huber: w_i = 1 if u_i <= k, else k / u_i.  Bisquare:
 *      w_i = (1 - (u_i / c)^2)^2 if u_i < c, else 0.  tune <= 0: k = 1.345, c = 4.685.
 *   5. Stopping test, once a solve has run and a previous x exists (X0 on a warm start; none after the first solve of a cold start):
 *      max_j |x_j - xold_j| <= tol max_j |x_j|: status 0, done.  Otherwise go to 3.
 * it counts solves and it <= maxit is the only loop bound; maxit <= 0 means 50.  A comparison with a NaN is false: a NaN in an included
 * row turns every weight into a NaN and the member leaves at the next count with info -2.  No input makes a loop run longer.
 *
 * Section 8's conventions hold: member q lives at base + q * stride, column-major, strides count elements; the plan supplies the stream
 * only; batch == 0 returns 0 after the argument checks and launches nothing.  A, b and the weights are never written.
 *
 * Outputs where info is 0: x; the robust weights w (m per member: those of the returned x's residuals, 1 for QR_LOSS_LS, for status 2
 * and on excluded rows); the scale s (0 for QR_LOSS_LS); resid = |b - A x|_2 over the included rows, unweighted; it; status 0
 * (converged, or QR_LOSS_LS), 2 (a zero scale) or 3 (maxit solves: x, w and s of the last iterate ARE written).
 *
 * dinfo[q]: 0; -1, -2 or i + 1 as above: nothing but info is written for such a member.  The other members are unaffected and the call
 * returns 0.  Dependence to rounding among the columns is NOT detected.
 *
 * Routes, chosen from the shape alone.  m <= 64 and n + 1 <= 32: one wave per member, four members per workgroup.  Otherwise one
 * workgroup per member with the image in LDS, for m <= qr_irls_batched_max_rows(n): the largest m <= 512 with
 * 8 ((n + 1) ld(m) + 3 m + 2 n + 72) bytes within 160 KiB, ld(m) the smallest value >= m that is 2 mod 32.  A member's results do not
 * depend on the batch size or on its place in the batch, and repeated calls are bitwise equal.  With QR_LOSS_LS and no weights x is
 * bitwise qr_gels_batched_dev's.
 *
 * Out of scope: several right-hand sides per member; m < n; other losses (L1, Cauchy); Huber's proposal 2; leverage and covariance
 * outputs; bounds or equalities combined with a robust loss; updating the factorisation between reweightings; a single-matrix variant;
 * blocked or MFMA variants.
 * ------------------------------------------------------------------------------------------- */
#define QR_LOSS_LS 0          /* weighted least squares */
#define QR_LOSS_HUBER 1       /* Huber loss */
#define QR_LOSS_BISQUARE 2    /* Tukey bisquare loss */

/* the largest m taken for n unknowns (at most 512); 0 if n is not taken (n < 1 or n > QR_BATCHED_MAX_N - 1).  No device is touched. */
int qr_irls_batched_max_rows(int n);

/* loss: QR_LOSS_*; tune: the constant k or c (<= 0: the default; NaN or inf: QR_E_ARG).  dA: m x n (lda >= m, strideA >= lda * n); dB: m
 * per member (strideB >= m); dprior: m per member, strideprior apart (0: one vector shared by all members, else >= m), NULL: ones;
 * dscale_in: one per member, NULL: the MAD scale; dX0: n per member (strideX0 >= n), NULL: a cold start (not referenced for QR_LOSS_LS);
 * tol >= 0; dX: n per member (strideX >= n); dW (may be NULL): m per member (strideW >= m); dscale, dresid, diter, dstatus (may be
 * NULL) and dinfo: one per member.  QR_E_ARG, before any device is touched, for a shape or an operand outside these rules (strideprior
 * is checked even when dprior is NULL). */
int qr_irls_batched_dev(qr_plan* plan, int loss, double tune,
                        const double* dA, int m, int n, int lda, long long strideA,
                        const double* dB, long long strideB,
                        const double* dprior, long long strideprior,
                        const double* dscale_in,
                        const double* dX0, long long strideX0,
                        double tol, int maxit,
                        double* dX, long long strideX,
                        double* dW, long long strideW,
                        double* dscale, double* dresid, int* diter, int* dstatus,
                        int* dinfo, int batch);

/* Weighted least squares, min sum_i p_i (b - A x)_i^2: qr_irls_batched_dev with QR_LOSS_LS.  dresid (may be NULL): |b - A x|_2 over
 * the rows with p_i > 0, unweighted. */
int qr_gels_weighted_batched_dev(qr_plan* plan,
                                 const double* dA, int m, int n, int lda, long long strideA,
                                 const double* dB, long long strideB,
                                 const double* dprior, long long strideprior,
                                 double* dX, long long strideX,
                                 double* dresid, int* dinfo, int batch);

/* The same as qr_irls_batched_dev for a packed batch on host pointers (A: m x n, b: m, prior: m, scale_in: 1, x0: n per member; prior,
 * scale_in and x0 may be NULL; all untouched): X n and W m per member, scale, resid, iter, status and info one per member (W, scale,
 * resid, iter and status may be NULL); the outputs of a member with a non-zero info read 0.  Returns QR_E_SINGULAR if any info word is
 * non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_robust_batched(const double* A, int m, int n, const double* b, int loss, double tune, const double* prior,
                            const double* scale_in, const double* x0, double tol, int maxit, int batch,
                            double* X, double* W, double* scale, double* resid, int* iter, int* status, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8k. Batched covariance, standard errors and leverages: what says how good the fits of 8 to 8j are.  For the weighted problem of 8j
 * (P = diag(p)) the calls give the parameter covariance sigma2 (A^T P A)^-1 and its standard errors, the residuals and the variance
 * estimate sigma2 = sum_i p_i e_i^2 / dof, the leverages h_i = p_i a_i^T (A^T P A)^-1 a_i, and the same quadratic form for new points
 * (the prediction variance).  MINPACK ships covar beside qrsolv and lmpar (8f, 8g); this is covar for a batch.
 *
 * Everything is computed from the triangle R of a QR factorisation, A^T P A = R^T R (with column pivoting: of A P_c), and R^T R is
 * never formed: the errors are of order kappa(A) eps, not kappa^2.  With r the rank and R11 the leading r x r block:
 *   T = R11^-1   along the rows, T R11 = I: s = (i == j ? 1 : 0), s = fma(-T(i,k), R(k,j), s) for k ascending, T(i,j) = s / R(j,j)
 *   C            mult * S(i,j), S(i,j) = sum over k = max(i,j) .. r-1 ascending of fma(T(i,k), T(j,k), .), scattered through jpvt:
 *                C = mult P [ (R11^T R11)^-1 0 ; 0 0 ] P^T, the covariance of the basic solution as MINPACK's covar defines it.  C is
 *                stored as a full symmetric matrix, both triangles from the one computed value (bitwise symmetric); the rows and columns
 *                of the dropped variables are exact zeros; se_j = sqrt(C_jj) of the stored value
 *   h_i          p_i |R11^-T (P^T a_i)(0 : r)|^2: per row one forward substitution with R^T, one fma per term in ascending index order,
 *                the squares added in ascending order; no inverse is formed.  A row with p_i == 0 gives exactly 0 and is not used
 *                (it may hold NaN).  This costs n^2 / 2 fmas per row where going through an explicit Q costs a second factorisation's
 *                worth of reflections; the price is an error of order kappa eps in h where Q gives n eps
 * A result does not depend on which call or kernel computed it: the fused call below returns bitwise what the from-factor calls return
 * on the same triangle.
 *
 * Section 8's conventions hold: member q lives at base + q * stride, column-major, strides count elements; the plan supplies the stream
 * only; QR_E_ARG for bad arguments before any device is touched; batch == 0 returns 0 after the argument checks and launches nothing;
 * inputs are never written; no scratch memory, no host wait, one launch per call.  Failure is per member and all or nothing: a non-zero
 * info word means nothing else was written for that member; the other members are unaffected and the call returns 0.  A member's results
 * do not depend on the batch size or on its place in the batch, and repeated calls are bitwise equal.
 *
 * Dependence to rounding among the columns is NOT detected by the fused call (only an exactly zero R(i,i)).  The pivoted path is
 * qr_geqp3_batched_dev -> qr_rank_batched_dev -> qr_covar_batched_dev and qr_leverage_batched_dev with that jpvt and rank.
 *
 * Out of scope: several right-hand sides per member; m < n; sandwich (robust) covariance, and the covariance of 8j's robust fits beyond
 * passing p w as the prior; leave-one-out, studentised residuals and Cook's distance (elementwise in e, h and sigma2); effective degrees
 * of freedom of the damped fits; covariance under the constraints of 8h and 8i; a single-matrix variant; blocked or MFMA variants.
 * ------------------------------------------------------------------------------------------- */
#define QR_COV_UNSCALED 0     /* C = (A^T P A)^-1 */
#define QR_COV_SCALED 1       /* C = sigma2 (A^T P A)^-1 */

/* the largest m qr_gels_stats_batched_dev takes for n unknowns: the largest m <= 512 with 8 ((n + 1) ld(m) + n + 72) bytes within
 * 160 KiB, ld(m) the smallest value >= m that is 2 mod 32 (512 for n <= 31; 256 x 63 fits); 0 if n is not taken (n < 1 or
 * n > QR_BATCHED_MAX_N - 1).  No device is touched. */
int qr_stats_batched_max_rows(int n);

/* MINPACK covar from a triangle that exists.  dR: the upper triangle of an n x n block per member (1 <= n <= QR_BATCHED_MAX_N, ldr >= n,
 * strideR >= ldr * n); the strict lower triangle is never read, so the in-place factors of qr_geqrf_batched_dev / qr_geqp3_batched_dev
 * (ldr = lda, strideR = strideA) and an accumulator's R can be passed as they are.  djpvt (0-based, n per member, stridejpvt >= n),
 * drank and dmult (one per member) may be NULL: the identity, n and 1.  dC (n x n, ldc >= n, strideC >= ldc * n) and dse (n per member,
 * stridese >= n): either may be NULL, not both.  dinfo: 0; i + 1 for the smallest i < rank with R(i,i) == 0 exactly; -1 for a jpvt that
 * is no permutation of 0 .. n-1, a rank outside 0 .. n or a multiplier that is negative, NaN or inf.  Rank 0 is valid: C = 0.
 * One wave per member for n <= 32 (four members per workgroup; the rows of T in registers), one workgroup per member above (R inverted
 * in place in LDS). */
int qr_covar_batched_dev(qr_plan* plan, const double* dR, int n, int ldr, long long strideR,
                         const int* djpvt, long long stridejpvt, const int* drank, const double* dmult,
                         double* dC, int ldc, long long strideC, double* dse, long long stridese,
                         int* dinfo, int batch);

/* dH[i] = p_i |R11^-T (P^T a_i)(0 : r)|^2 for the mrows rows of dA (mrows x n, lda >= mrows, strideA >= lda * n; any mrows >= 1: the
 * fitted rows or new points), the triangle, djpvt and drank as above.  dprior: mrows per member, strideprior apart (0: one vector shared
 * by all members, else >= mrows; checked even when dprior is NULL), NULL: ones.  dH: mrows per member (strideH >= mrows).  dinfo: 0;
 * i + 1 for a zero diagonal entry; -1 for a bad jpvt, a bad rank, or a prior weight that is negative, NaN or inf (in any row: no row of
 * such a member is written).  One workgroup per member and 256 rows, one row per thread; batch * ceil(mrows / 256) must fit an int.
 * With dprior given, every workgroup of a member reads ALL its mrows weights before it writes (that is what keeps a bad weight in any
 * row from leaving other rows of the member written): mrows^2 / 256 reads per member.  That is nothing at a few thousand rows and
 * about 4e9 reads at mrows = 1e6: a caller with very many rows per member feeds them in calls of some ten thousand rows each, which
 * return the same values row by row. */
int qr_leverage_batched_dev(qr_plan* plan, const double* dR, int n, int ldr, long long strideR,
                            const int* djpvt, long long stridejpvt, const int* drank,
                            const double* dA, int mrows, int lda, long long strideA,
                            const double* dprior, long long strideprior,
                            double* dH, long long strideH, int* dinfo, int batch);

/* The fit of qr_gels_weighted_batched_dev and its statistics in ONE launch: A m x n, n <= m <= qr_stats_batched_max_rows(n), one b,
 * prior weights as in 8j (p_i = 0 excludes a row, which may hold NaN).  cnt = the rows with p_i > 0, dof = cnt - n.  Outputs where
 * info is 0 (every one but dX and dinfo may be NULL): dX (n; bitwise qr_gels_weighted_batched_dev's); dE (m): e = b - A x from the
 * untouched inputs, one fma per term, exact 0 on excluded rows; dH (m): the leverages; dsigma2 = sum p_i e_i^2 / dof (+inf when
 * dof == 0) and ddof (int); dC (n x n) and dse (n): (A^T P A)^-1 for QR_COV_UNSCALED, sigma2 times it for QR_COV_SCALED, as
 * qr_covar_batched_dev computes them from the fit's R with dmult NULL or sigma2.  dinfo: 0; -1 a prior weight that is negative, NaN or
 * inf; -2 cnt < n; -3 QR_COV_SCALED with dof == 0; i + 1 an exactly zero R(i,i).  Routes as in 8j: a wave per member for m <= 64 and
 * n + 1 <= 32, else a workgroup per member with the image in LDS; R is inverted in place in the top of the image. */
int qr_gels_stats_batched_dev(qr_plan* plan, int scaled,
                              const double* dA, int m, int n, int lda, long long strideA,
                              const double* dB, long long strideB,
                              const double* dprior, long long strideprior,
                              double* dX, long long strideX,
                              double* dE, long long strideE,
                              double* dH, long long strideH,
                              double* dsigma2, int* ddof,
                              double* dC, int ldc, long long strideC,
                              double* dse, long long stridese,
                              int* dinfo, int batch);

/* qr_covar_batched_dev on a batched accumulator's R (section 8d), the multiplier formed on the device: sigma2 = rss[rhs] / (rows - n)
 * (+inf when rows == n), written to dsigma2 (one per member, may be NULL); C = (R^T R)^-1 for QR_COV_UNSCALED, sigma2 times it for
 * QR_COV_SCALED.  dinfo (acc's batch ints): 0; i + 1 for a member that holds fewer than n rows (the first zero R(i,i)); -3 for
 * QR_COV_SCALED with rows == n; -1 for QR_COV_SCALED where sigma2 is no finite number >= 0 (a NaN or inf that was pushed sits in
 * rss).  The state is untouched.  No host wait. */
int qr_lsacc_batched_covar_dev(qr_lsacc_batched* acc, int scaled, int rhs,
                               double* dC, int ldc, long long strideC, double* dse, long long stridese,
                               double* dsigma2, int* dinfo);

/* qr_gels_stats_batched_dev for a packed batch on host pointers (A: m x n, b: m, prior: m per member; prior may be NULL; all untouched):
 * X n, E and H m, sigma2 and dof one, Cov n x n (ld n) and se n per member (all but X and info may be NULL); the outputs of a member
 * with a non-zero info read 0.  Returns QR_E_SINGULAR if any info word is non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_stats_batched(const double* A, int m, int n, const double* b, const double* prior, int scaled, int batch,
                           double* X, double* E, double* H, double* sigma2, int* dof, double* Cov, double* se, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8l. Batched inequality-constrained least squares (Lawson & Hanson's LSEI): for every member of a batch
 *
 *         min |A x - b|_2  subject to  G(0:neq, :) x = h(0:neq),  G(neq:mg, :) x >= h(neq:mg),
 *
 * A: m x n, G: mg x n, 0 <= neq <= min(n, mg), 1 <= mg <= 64, 1 <= n <= QR_BATCHED_MAX_N - 1, m >= 1, m + neq >= n, one b per member --
 * what 8i leaves out: a joint limit expressed in task space, friction-cone facets, half-space collision avoidance, a monotone or convex
 * fit, an interpolation condition together with a sign constraint.  neq == mg is 8h's problem; bounds are rows +-e_j^T of G.  The
 * active-set loop of every member runs on the device: one launch whatever the batch size; nothing waits on the host.
 *
 * The method is a dual active-set loop whose every candidate is 8h's null-space solve (the textbook reduction LSI -> LDP -> NNLS is not
 * used: it loses the constraints to kappa eps on graded columns).  Per member the state is the working set W (rows < neq are in it for
 * good), mu (mg entries), x, a ban set and the count it.  A candidate of a row set S is the solution of min |A x - b| subject to
 * G_S x = h_S by steps 1 to 8 of 8h (a plain factorisation and solve of A when S is empty): x_S and zeta = -lambda_S, so that
 * A^T (A x_S - b) = G_S^T zeta.  The rows of S are taken in ascending index order, a pending row t last.
 *   1. Start.  W = {0 .. neq-1}; it = 1; (x, mu_W) = candidate(W).  An exactly zero R_c(i,i) gives info -3; an exactly zero R_a(i,i),
 *      here or in any later candidate, gives info i + 1; in both cases nothing else is written.
 *   2. Outer test.  s = G x - h from the untouched G.  Among the rows i >= neq outside W and not banned the most negative s_i, ties to
 *      the smallest index.  None < 0: done, info 0.  Otherwise t is that row, mu_t = 0, pend = true.
 *   3. Count.  it == maxit: done, info n + 1, the last accepted (x, mu) is written.  Otherwise ++it.
 *   4. Dependence.  [G_W^T | G_t^T] is factored over its first |W| columns, the last riding along; rho is the norm of that column's rows
 *      |W| .. n-1.  If |W| == n or rho <= rcond |G_t|_2: c = R_c^-1 (its top |W| entries); over the i in W with i >= neq and c_i > 0,
 *      theta = min mu_i / c_i, ties to the smallest index k.  No such i: info -2 (infeasible), nothing else written.  Otherwise
 *      mu_W -= theta c, mu_t += theta, mu_k = 0 exactly and k leaves W, every other inequality member with mu <= 0 is set to 0 and
 *      leaves; pend = false; go to 3.  Otherwise the same factorisation is completed with t's column: nothing is factored twice.
 *   5. Candidate.  (x_c, zeta) = candidate(W + {t}).
 *   6. Anti-cycling, only when pend is set, which it clears: zeta_t <= 0: t is banned, mu_t = 0, go to 2.
 *   7. Accept.  zeta_i > 0 for every inequality i in W + {t}: W gains t, mu = zeta on W and 0 elsewhere, x = x_c, the bans are
 *      lifted, go to 2.
 *   8. Blocked step.  Over the inequality i in W + {t} with zeta_i <= 0, alpha = min mu_i / (mu_i - zeta_i), ties to the smallest index
 *      k.  k == t (this does not happen in exact arithmetic): nothing moves -- W and mu are those of the last accepted pair again --, t
 *      is banned, go to 2.  Otherwise mu_i += alpha (zeta_i - mu_i) over W + {t}, equalities included; mu_k = 0 exactly and k leaves
 *      W; every other inequality member with mu <= 0 is set to 0 and leaves.  Go to 3 (t stays pending, pend stays false).
 * Every candidate is factored from scratch from the untouched inputs.  it counts every candidate and every dependence step, and
 * it <= maxit is the only loop bound; maxit <= 0 means 3 mg + 1.  rcond <= 0 means n eps, the size a dependent column's diagonal is left
 * at by a Householder factorisation of n rows.  A comparison with a NaN is false and leads towards the count.
 *
 * Section 8's conventions hold: member q lives at base + q * stride, column-major, strides count elements; the plan supplies the stream
 * only; batch == 0 returns 0 after the argument checks and launches nothing.  The inputs are never written.  strideG == 0 shares one G,
 * strideH == 0 one h, across the batch.
 *
 * Outputs: x of the last accepted candidate; mu of that candidate (zeta on its set: > 0 on the inequalities of the set, either sign on
 * the equalities, exactly 0 elsewhere); state (1 in the set, else 0); s = G x - h and resid = |A x - b| recomputed from the untouched
 * A, G and the returned x; iter, the count.
 *
 * dinfo[q]: 0 solved; n + 1 the count was reached: the last accepted pair IS written, with s showing what it still violates; -2
 * infeasible; -3 equalities exactly dependent; i + 1 an exactly zero R_a(i,i): nothing but info is written for the last three.  The
 * other members are unaffected and the call returns 0.  Dependence to rounding among the columns of A on a null space is NOT detected,
 * as in 8h.
 *
 * Routes, chosen from the shape alone.  m <= 64 and n + 1 <= 32: one wave per member, four members per workgroup.  Otherwise one
 * workgroup per member with the image of A and the factors of G_S^T in LDS, for m <= qr_lsei_batched_max_rows(n, mg): the largest
 * m <= 512 with 8 ((n + 1) ld(m) + (n + 1) ld(n) + 5 mg + 4 n + 72) bytes within 160 KiB, ld(r) the smallest value >= r that is 2 mod
 * 32.  A member's results do not depend on the batch size or on its place in the batch, and repeated calls are bitwise equal.  With
 * neq == mg x is bitwise qr_gglse_batched_dev's; where no row is ever violated x is bitwise qr_gels_batched_dev's.
 *
 * Out of scope: several right-hand sides per member; mg > 64; a warm start from a given set; updating factors across set changes; a
 * single-matrix variant; blocked or MFMA variants.
 * ------------------------------------------------------------------------------------------- */

/* the largest m taken for n unknowns and mg constraint rows (at most 512); 0 if (n, mg) is not taken (n < 1, n > QR_BATCHED_MAX_N - 1,
 * mg < 1 or mg > 64).  No device is touched. */
int qr_lsei_batched_max_rows(int n, int mg);

/* dA: m x n (lda >= m, strideA >= lda * n); dB: m per member (strideB >= m); dG: mg x n (ldg >= mg; strideG 0: one G shared by all
 * members, else >= ldg * n); dH: mg per member (strideH 0: shared, else >= mg); dX: n per member (strideX >= n); dMU, dS (may be NULL):
 * mg per member (strideMU, strideS >= mg); dstate (may be NULL): mg ints per member (stridestate >= mg); dresid, diter (may be NULL) and
 * dinfo: one per member.  QR_E_ARG, before any device is touched, for a shape or an operand outside these rules. */
int qr_lsei_batched_dev(qr_plan* plan,
                        const double* dA, int m, int n, int lda, long long strideA,
                        const double* dB, long long strideB,
                        const double* dG, int mg, int neq, int ldg, long long strideG,
                        const double* dH, long long strideH,
                        int maxit, double rcond,
                        double* dX, long long strideX,
                        double* dMU, long long strideMU,
                        double* dS, long long strideS,
                        int* dstate, long long stridestate,
                        double* dresid, int* diter,
                        int* dinfo, int batch);

/* The same for a packed batch on host pointers (A: m x n, b: m, G: mg x n, h: mg per member, all untouched): X n, MU, S and state mg
 * per member, resid, iter and info one per member (MU, S, state, resid and iter may be NULL); the outputs of a member with info -2, -3
 * or i + 1 read 0.  Returns QR_E_SINGULAR if any info word is non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_inequality_batched(const double* A, int m, int n, const double* b, const double* G, int mg, int neq, const double* h,
                                int maxit, double rcond, int batch,
                                double* X, double* MU, double* S, int* state, double* resid, int* iter, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8m. Batched Levenberg-Marquardt: MINPACK lmder's outer loop for every member of a batch,
 *
 *         min |f(x)|_2,      f: R^n -> R^m, m >= n, 1 <= n <= QR_BATCHED_MAX_N - 1, m <= qr_batched_max_rows(n + 1),
 *
 * with the Jacobian J(x) (m x n) supplied by the caller -- per-pixel curve fitting, damped inverse kinematics with a step limit, the users
 * sections 8f, 8g and 8k were built for (qrsolv, lmpar and covar; this is lmder around them).  The loop is split by reverse
 * communication into two device calls, so that the caller's model code runs between them on the same stream and no call but
 * qr_lm_batched_running waits on the host:
 *
 *     qr_lm_batched_start_dev(lm, dX0, ...);
 *     repeat:  fill J(x) and f(x) of every member at state.x;   qr_lm_batched_step_dev(lm, dJ, ..., dF, ...);
 *              fill f(xtrial) of every member at state.xtrial;  qr_lm_batched_update_dev(lm, dFtrial, ...);
 *              every few rounds: qr_lm_batched_running(lm, &count), until count == 0
 *
 * A member that the update rejected keeps its x, so the caller hands in the same J and f again and the factorisation returns the same
 * bits: one rule for every member, no branch on the host.  A member whose status or info word is not 0 is skipped by both kernels: what
 * the caller leaves in its slots of J and F is factored but never used, its state stays bitwise frozen, and its neighbours are
 * unaffected.  step twice in a row, update before a step and either before start return QR_E_ARG from a phase flag kept on the host.
 *
 * Layout: section 8's (member q at base + q * stride, column-major, strides in elements); the stride rules are section 8g's.  The plan
 * supplies the stream only.  QR_E_ARG for bad arguments before anything touches a device; batch == 0 is allowed (nothing is launched).
 *
 * The state (qr_lm_batched_view; packed per-member device arrays, read-only for the caller): x, xtrial, D (n each); delta, par (MINPACK's
 * par = lambda^2, not lambda), fnorm, xnorm = |D x|, pnorm = |D p|, gnorm, prered, dirder; iter, nfev, njev (the steps run), accepted
 * (0 / 1: what the last update did), status, info, par_status (section 8g's status of the last search).
 *   status: 0 running; MINPACK's info otherwise: 1 ftol, 2 xtol, 3 both, 4 gnorm <= gtol, 5 nfev >= maxfev, 6 ftol too small,
 *           7 xtol too small, 8 gtol too small; -1: the member has an info word from the search.
 *   info:   0; -1 for a D of mode 2 with an entry that is not > 0 (found by the first step: nothing else is written, status stays 0, and
 *           the member is skipped from then on) or for a radius that is no finite positive number; i + 1 for the smallest i with a zero
 *           on the diagonal of a damped triangle (section 8g's words; status is then -1).
 *
 * qr_lm_batched_step_dev: qr_geqp3_batched_dev's launch on dJ, qr_ormqr_batched_dev's 'T' launch on dF, then one new launch: dJ returns as
 * geqp3 leaves it and dF as Q^T f.  qr_lm_step_batched_dev is that one new launch alone for factors the caller already has (R, the top
 * zrows >= n rows of Q^T f, the sum of squares of the rows that are not there in drss, jpvt or NULL: section 8g's operand rules); the R
 * and Z of a batched accumulator qualify.  Per running member, with MINPACK's names:
 *   a. fnorm = sqrt(sum over all rows of (Q^T f)^2 (+ drss)), recomputed at every step by this one rule.  MINPACK takes |f| from f itself:
 *      the two are equal to rounding.
 *   b. acnorm[jpvt[k]] = |R(0:k, k)|, the norm of the column of J through its column of R.  MINPACK takes it from J before factoring: the
 *      two are equal to rounding.
 *   c. the member's first step: mode 1: D_j = acnorm_j, or 1 where that is 0; mode 2: D is qr_lm_batched_start_dev's; xnorm = |D x|;
 *      delta = factor * xnorm, or factor if that is 0.
 *   d. gnorm = max over k with acnorm != 0 of |sum_{i<=k} R(i,k) (z_i / fnorm)| / acnorm[jpvt[k]], 0 if fnorm == 0; gnorm <= gtol: status 4.
 *   e. mode 1: D = max(D, acnorm).
 *   f. section 8g's search (the same device code: p, par, pnorm and par_status are bitwise qr_trust_batched_dev's on the same factors, D,
 *      delta and start) from par, with par_rtol and par_maxit.
 *   g. xtrial = x - p; while iter == 1 (no step accepted yet): delta = min(delta, pnorm).
 *   h. temp1 = |R P^T p| / fnorm (each row's sum over the columns ascending), temp2 = sqrt(par) pnorm / fnorm.
 *   i. prered = temp1^2 + temp2^2 / 0.5, dirder = -(temp1^2 + temp2^2), njev += 1.
 * qr_lm_batched_update_dev, per running member: fnorm1 = |ftrial|; actred = 1 - (fnorm1 / fnorm)^2 if 0.1 fnorm1 < fnorm, else -1 (a
 * fnorm1 that is NaN or inf counts as -1: an addition to MINPACK, such a trial point is rejected and delta shrinks); ratio = actred /
 * prered (0 if prered == 0); lmder's rules for delta and par (the ratio <= 0.25 branch with temp, its 0.1 floor, delta = temp min(delta,
 * pnorm / 0.1), par /= temp; the par == 0 or ratio >= 0.75 branch); acceptance at ratio >= 1e-4 (x = xtrial, xnorm = |D x|, fnorm =
 * fnorm1, iter += 1); nfev += 1; the stopping tests in MINPACK's order (1, 2, 3, then 5, 6, 7, 8).
 *
 * Routes, by shape alone: the step is a wave per member (four per workgroup, no barrier) for n + 1 <= 32, else a workgroup per member;
 * the update is a wave per member.  No atomics, every sum in a fixed order: a member's results do not depend on the batch size or on its
 * place in the batch, and repeats are bitwise equal.
 *
 * Out of scope: a fused factor-and-step launch on the wave route; lmdif's finite-difference Jacobian; bounds or constraints on x;
 * m < n; skipping the refactorisation of rejected members; several residual vectors per member.
 * ------------------------------------------------------------------------------------------- */
typedef struct qr_lm_batched qr_lm_batched;

typedef struct {
    double ftol, xtol, gtol, factor, par_rtol;
    int maxfev, mode, par_maxit;
} qr_lm_options;

typedef struct {
    double *x, *xtrial, *D, *delta, *par, *fnorm, *xnorm, *pnorm, *gnorm, *prered, *dirder;
    int *iter, *nfev, *njev, *accepted, *status, *info, *par_status;
} qr_lm_batched_state;

/* the host-pointer twin's model: what = 1: F (batch x m, member after member) <- f at X (batch x n); 2: J (batch matrices m x n,
 * column-major) <- the Jacobian at X; 3: F <- f at X, X being the trial points.  A non-zero return stops the solve and is returned. */
typedef int (*qr_lm_fcn)(void* user, int what, const double* X, int batch, double* F, double* J);

/* MINPACK lmder1's: ftol = xtol = sqrt(DBL_EPSILON), gtol = 0, factor = 100, mode = 1, par_rtol = 0.1, par_maxit = 10; maxfev = 0 stands
 * for 100 (n + 1) */
void qr_lm_options_default(qr_lm_options* opt);

/* opt NULL: the defaults.  QR_E_ARG for ftol, xtol or gtol < 0, factor <= 0, mode not 1 or 2, par_rtol outside (0, 1), par_maxit < 1,
 * maxfev < 0 (NaN anywhere included) and for a shape outside the rules above. */
int qr_lm_batched_create(qr_lm_batched** lm, qr_plan* plan, int m, int n, int batch, const qr_lm_options* opt);
/* dX0: n per member (ldx >= n, strideX >= ldx); dD0: the scaling of mode 2, n per member (strideD 0: shared, else >= n), not read in mode 1 */
int qr_lm_batched_start_dev(qr_lm_batched* lm, const double* dX0, int ldx, long long strideX, const double* dD0, long long strideD);
/* dJ: m x n (ldj >= m, strideJ >= ldj * n), dF: m per member (ldf >= m, strideF >= ldf) */
int qr_lm_batched_step_dev(qr_lm_batched* lm, double* dJ, int ldj, long long strideJ, double* dF, int ldf, long long strideF);
int qr_lm_batched_update_dev(qr_lm_batched* lm, const double* dFtrial, int ldf, long long strideF);
int qr_lm_batched_view(qr_lm_batched* lm, qr_lm_batched_state* state);
/* count <- the members with status == 0 and info == 0.  The one call that waits on the host. */
int qr_lm_batched_running(qr_lm_batched* lm, int* count);
int qr_lm_batched_destroy(qr_lm_batched* lm);

/* The step from factors that exist, in qr_lm_batched_step_dev's place in the protocol: dR n x n (ldr >= n, strideR >= ldr * n; the upper
 * triangle is read), dZ zrows x 1 (n <= zrows <= ldz <= strideZ), drss (one per member, may be NULL: 0), djpvt (n per member,
 * stridejpvt >= n; NULL: the identity). */
int qr_lm_step_batched_dev(qr_lm_batched* lm, const double* dR, int ldr, long long strideR, const double* dZ, int zrows, int ldz,
                           long long strideZ, const double* drss, const int* djpvt, long long stridejpvt);

/* The whole solve of a packed batch on host pointers: X (batch x n) holds the starts on entry and the results on return; D: the scaling
 * of mode 2 (batch x n), else NULL; fnorm, nfev, njev, status (may be NULL) and info: one per member.  fcn is called on host buffers.
 * Returns QR_E_SINGULAR if any info word is non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_lm_batched(qr_lm_fcn fcn, void* user, int m, int n, int batch, double* X, const double* D, const qr_lm_options* opt,
                        double* fnorm, int* nfev, int* njev, int* status, int* info);

/* ---------------------------------------------------------------------------------------------
 * 8n. Batched Levenberg-Marquardt with box bounds on x: section 8m's loop for every member of a batch,
 *
 *         min |f(x)|_2  subject to  lo <= x <= hi,      shapes as in section 8m,
 *
 * for the users of section 8m whose parameters have simple bounds: an amplitude >= 0, a width > 0, a joint inside its limits, a parameter
 * held fixed (lo_j == hi_j).  Entries of lo and hi may be -inf and +inf.  Clipping the trial point between section 8m's two calls is the
 * wrong answer (its prered then belongs to a step that was not taken); the rules below sit inside the step.  They are MPFIT's (Markwardt's
 * extension of MINPACK to bounds) with two corrections, marked (*).  The protocol, the phase flag, the layout, the stride rules, the
 * options and the routes are section 8m's, with its words; section 8m itself is unchanged, and with every bound infinite every state array
 * below is bitwise section 8m's after every call (both run the same device code).
 *
 *     qr_lmb_batched_start_dev(lm, dX0, ..., dLo, ..., dHi, ...);
 *     repeat:  fill J(x) and f(x) at state.x;      qr_lmb_batched_step_dev(lm, dJ, ..., dF, ...);
 *              fill f(xtrial) at state.xtrial;     qr_lmb_batched_update_dev(lm, dFtrial, ...);
 *              every few rounds: qr_lmb_batched_running(lm, &count), until count == 0
 *
 * The state (qr_lmb_batched_view): section 8m's fields, then lo, hi (n each), peg (n ints: -1 held at lo, +1 held at hi, 0 free), alpha
 * (the fraction of the search's step that was taken) and clipped (1: alpha < 1).
 *   info: section 8m's words, and -2 from qr_lmb_batched_start_dev for a member whose bounds are no box (lo_j > hi_j, or a NaN) or whose
 *         x0 lies outside the box: nothing else of the member is written, and it is skipped from then on.
 *
 * qr_lmb_batched_step_dev: four launches: peg, qr_geqp3_batched_dev's, qr_ormqr_batched_dev's, the step.  Per running member, x_new = x - p:
 *   P. peg, on the unfactored J and f: g_j = sum_i J(i, j) f_i for the columns whose x_j is exactly on a bound (a fixed order of summation);
 *      peg_j = -1 if x_j == lo_j and g_j > 0, +1 if x_j == hi_j and g_j < 0, else 0.  The held columns of dJ are overwritten with zeros; the
 *      factorisation then runs unchanged.  A zero column has acnorm 0, so rules b to e of section 8m need no change: D_j = 1 at a first
 *      step, the column is left out of gnorm (gnorm is the scaled projected gradient), and a member whose every column is held ends with
 *      status 4.
 *   S. the step, between rules f and g of section 8m: s = -p; s_j = 0 exactly for every held j (*: rounding must not move a held variable
 *      off its bound); s_j = 0 where x_j <= lo_j and s_j < 0, and where x_j >= hi_j and s_j > 0; alpha = min(1, the smallest
 *      (bound_j - x_j) / s_j over the j with s_j != 0 whose x_j + s_j leaves the box); p~ = -alpha s; xtrial_j = x_j - p~_j clamped to
 *      [lo_j, hi_j], and the bound itself, bitwise, for every j whose ratio equals alpha.  If nothing was zeroed and alpha == 1, rules g, h
 *      and i hold verbatim.  Otherwise, with g_k the gradient entries of rule d: temp1 = |R P^T p~| / fnorm, prered = max(0, 2 sum_k p~_k g_k
 *      / fnorm - temp1^2), dirder = -sum_k p~_k g_k / fnorm: the linear model's own reduction for the step taken.  pnorm stays the search's
 *      |D p| in every case (*: with the truncated length the update's delta = pnorm / 0.5 collapses the radius onto the bound).
 * qr_lmb_batched_update_dev: section 8m's update; while clipped is set the two tests on the reductions (status 1 and 6) are left out: a tiny
 * alpha makes actred and prered tiny without meaning convergence.
 *
 * A variable that is free on its bound and whose step points outward is zeroed; if the trial is then rejected, the shrinking radius turns
 * p towards -D^-2 g, which by rule P points inward for that variable: no list of banned variables is kept.
 *
 * Out of scope: the step from factors that already exist (section 8m's qr_lm_step_batched_dev has no bounded twin: the peg reads the
 * unfactored J); general linear constraints on x; m < n.
 * ------------------------------------------------------------------------------------------- */
typedef struct qr_lmb_batched qr_lmb_batched;

typedef struct {
    double *x, *xtrial, *D, *delta, *par, *fnorm, *xnorm, *pnorm, *gnorm, *prered, *dirder;
    int *iter, *nfev, *njev, *accepted, *status, *info, *par_status;
    double *lo, *hi, *alpha;
    int *peg, *clipped;
} qr_lmb_batched_state;

/* the options and the shape rules are qr_lm_batched_create's */
int qr_lmb_batched_create(qr_lmb_batched** lm, qr_plan* plan, int m, int n, int batch, const qr_lm_options* opt);
/* dX0 and dD0 as in qr_lm_batched_start_dev; dLo, dHi: n per member (stride 0: one vector shared by all members, else >= n); either may
 * be NULL: that side is unbounded */
int qr_lmb_batched_start_dev(qr_lmb_batched* lm, const double* dX0, int ldx, long long strideX, const double* dD0, long long strideD,
                             const double* dLo, long long strideLo, const double* dHi, long long strideHi);
/* dJ: m x n (ldj >= m, strideJ >= ldj * n), dF: m per member (ldf >= m, strideF >= ldf).  dJ returns as geqp3 leaves it (the held columns
 * factored as zeros), dF as Q^T f */
int qr_lmb_batched_step_dev(qr_lmb_batched* lm, double* dJ, int ldj, long long strideJ, double* dF, int ldf, long long strideF);
int qr_lmb_batched_update_dev(qr_lmb_batched* lm, const double* dFtrial, int ldf, long long strideF);
int qr_lmb_batched_view(qr_lmb_batched* lm, qr_lmb_batched_state* state);
/* count <- the members with status == 0 and info == 0.  The one call that waits on the host. */
int qr_lmb_batched_running(qr_lmb_batched* lm, int* count);
int qr_lmb_batched_destroy(qr_lmb_batched* lm);

/* The whole solve of a packed batch on host pointers, as qr_lstsq_lm_batched: lo, hi (batch x n; either may be NULL: unbounded).  The X of
 * a member with info -2 returns as it came.  Returns QR_E_SINGULAR if any info word is non-zero.  Creates a plan of its own.  Synchronous. */
int qr_lstsq_lm_bounded_batched(qr_lm_fcn fcn, void* user, int m, int n, int batch, double* X, const double* lo, const double* hi,
                                const double* D, const qr_lm_options* opt, double* fnorm, int* nfev, int* njev, int* status, int* info);

#ifdef __cplusplus
}
#endif
#endif
