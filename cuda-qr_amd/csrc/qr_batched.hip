// qr_batched.hip -- kernels of the batched interface (qr_batched.c, mi355x_qr.h section 8): many small matrices, one per wave or workgroup.
//
//   b_wave_kernel<W>   m <= 64, at most W <= 32 columns: one wave per matrix, four matrices per workgroup.  Lane i holds row i in W
//                      registers; norms and dot products are wave butterflies; no barrier, no LDS in the factorisation
//   b_wg_kernel        everything else within qr_batched_max_rows: one workgroup per matrix, the matrix resident in LDS at a leading
//                      dimension of 2 mod 32 (the column loop of tp_panel_kernel, qr_update.hip, with no triangle on top); the trailing
//                      update is rank-1, one wave per column
//   b_ormqr_kernel     Q^T C / Q C, V resident in LDS, one wave per column of C with the column in registers
//   b_eye_kernel       the thin identity (qr_orgqr_batched_dev = this + b_ormqr_kernel 'N')
//   b_trsm_kernel      R X = B per matrix, one thread per right-hand side, and the info word (the composed route of gels)
//   bp_*               the same with column pivoting (section 8b), further down
//
// The Householder column step of either route, the solves and the wave helpers are qr_batched_dev.h's (qb_*), shared with the pivoted
// kernels below and with qr_batched_minnorm.hip; a kernel adds its loads and stores, its tau store and what it does between steps.
//
// Both factorisation kernels take `nrhs` extra columns from B that are updated but never factored (the fused gels: B <- Q^T B) and
// then run the back substitution in the same launch.  LAPACK dgeqr2 / dlarfg per column: beta = -sign(alpha) hypot(alpha,
// |x|), tau = (beta - alpha) / beta, v = x / (alpha - beta); x == 0 exactly: tau = 0, the column unchanged.
//
// Every sum runs in a fixed order that depends on (m, n, nrhs) alone (wave butterflies, waves added in wave order, serial loops):
// repeated launches are bitwise equal and a matrix's result does not depend on the batch count or its index.  No atomics.
#include "qr_batched_dev.h"

#define B_MAXN QRD_B_MAX_N

static_assert(QRD_B_MAX_N == 64, "the routes below assume at most 64 columns in LDS");

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  Dynamic LDS is used by the fused solve only: per wave R (W x (W + 1)) and the right-hand sides (W x (W + 1)).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) b_wave_kernel(double* __restrict__ A, int m, int n, int lda, size_t strideA, double* __restrict__ tau,
                                                     size_t stridetau, double* __restrict__ B, int nrhs, int ldb, size_t strideB,
                                                     int* __restrict__ info, int batch)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;          // (no barrier below: the waves of a workgroup are independent)
    double* Aq = A + q * strideA;
    double* Bq = nrhs ? B + q * strideB : nullptr;
    const int ntot = n + nrhs;
    const bool row = lane < m;
    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (row && c < n) v = Aq[(size_t) c * lda + lane];
        else if (row && c < ntot) v = Bq[(size_t) (c - n) * ldb + lane];
        a[c] = v;
    }
    double tauv = 0.0, diag = 1.0;            // lane j: tau[j] and R(j, j)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) qb_wave_col<W>(a, j, ntot, lane, tauv, diag);      // (wave-uniform; B's columns ride along)
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (row && c < n) Aq[(size_t) c * lda + lane] = a[c];
    if (lane < n) tau[q * stridetau + lane] = tauv;
    if (!nrhs) return;
    const int inf = qb_info_wave(diag, n, lane);
    if (lane == 0) info[q] = inf;
    if (inf) {                                // B <- Q^T B, no solve
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (row && c >= n && c < ntot) Bq[(size_t) (c - n) * ldb + lane] = a[c];
        return;
    }
    // staging: rows 0 .. n-1 of R and of Q^T B into this wave's LDS, the rest of Q^T B straight back
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;       // Rs[c * LW + r] = R[r, c]
    double* Xs = Rs + W * LW;                          // Xs[r * LW + k] = (Q^T B)[k, r], then X
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            if (lane < n) Rs[c * LW + lane] = a[c];
        } else if (c < ntot) {
            if (lane < n) Xs[(c - n) * LW + lane] = a[c];
            else if (row) Bq[(size_t) (c - n) * ldb + lane] = a[c];
        }
    }
    QB_WAVE_SYNC();
    if (lane < nrhs) qb_trsv(Rs, LW, n, Xs + lane * LW);      // (nrhs < W <= 32: one lane per right-hand side)
    QB_WAVE_SYNC();
    for (int r = 0; r < nrhs; ++r)
        if (lane < n) Bq[(size_t) r * ldb + lane] = Xs[r * LW + lane];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = column c of [A | B], ld = qb_ld(m); then red[4], a word for info, 3 spare.
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ size_t b_wg_lds(int m, int ntot) { return sizeof(double) * ((size_t) ntot * qb_ld(m) + 8); }

__global__ void __launch_bounds__(256) b_wg_kernel(double* __restrict__ A, int m, int n, int lda, size_t strideA, double* __restrict__ tau,
                                                   size_t stridetau, double* __restrict__ B, int nrhs, int ldb, size_t strideB,
                                                   int* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = qb_ld(m), ntot = n + nrhs;
    double* As = sm;
    double* red = As + (size_t) ntot * ld;
    int* sinfo = (int*) (red + 4);
    double* Aq = A + q * strideA;
    double* Bq = nrhs ? B + q * strideB : nullptr;
    double* tq = tau + q * stridetau;
    for (int c = wv; c < ntot; c += 4) {
        const double* src = c < n ? Aq + (size_t) c * lda : Bq + (size_t) (c - n) * ldb;
        for (int i = lane; i < m; i += 64) As[c * ld + i] = src[i];
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double tj = qb_wg_col(As, ld, m, j, ntot, red, t);
        if (t == 0) tq[j] = tj;
        __syncthreads();                      // (red and column j are read no more)
    }
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < m; i += 64) Aq[(size_t) c * lda + i] = As[c * ld + i];
    if (!nrhs) return;
    if (t == 0) info[q] = *sinfo = qb_info_serial(As, ld, n);
    __syncthreads();
    if (*sinfo == 0) {
        if (t < nrhs) qb_trsv(As, ld, n, As + (size_t) (n + t) * ld);         // (nrhs < 64: one thread per right-hand side)
        __syncthreads();
    }
    for (int c = n + wv; c < ntot; c += 4)
        for (int i = lane; i < m; i += 64) Bq[(size_t) (c - n) * ldb + i] = As[c * ld + i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// C <- Q^T C (tr != 0) or Q C.  LDS: Vs[c * ld + i] = V[i, c] below the diagonal, then tau[n].  A wave takes a column of C with row
// lane + 64 k in register k -- RR = 1, 2, 4 or 8 registers, the smallest that holds m rows --, reflectors in order 0 .. n-1 (Q^T) or
// n-1 .. 0 (Q).  (A row register beyond m would only add exact zeros: the result does not depend on RR.)
// ---------------------------------------------------------------------------------------------------------------------------------
#define B_ROWREGS 8
static_assert(QRD_B_MAX_ROWS <= 64 * B_ROWREGS, "a column of C is held in B_ROWREGS registers per lane");

__host__ __device__ __forceinline__ size_t b_ormqr_lds(int m, int n) { return sizeof(double) * ((size_t) n * qb_ld(m) + B_MAXN); }

template <int RR>
__global__ void __launch_bounds__(256) b_ormqr_kernel(int tr, const double* __restrict__ A, int m, int n, int lda, size_t strideA,
                                                      const double* __restrict__ tau, size_t stridetau, double* __restrict__ Cm, int nrhs,
                                                      int ldc, size_t strideC)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = qb_ld(m);
    double* Vs = sm;
    double* ts = Vs + (size_t) n * ld;
    const double* Aq = A + q * strideA;
    double* Cq = Cm + q * strideC;
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < m; i += 64) Vs[c * ld + i] = Aq[(size_t) c * lda + i];
    if (t < n) ts[t] = tau[q * stridetau + t];
    __syncthreads();
    for (int col = (int) blockIdx.y * 4 + wv; col < nrhs; col += (int) gridDim.y * 4) {       // (wave-uniform)
        double* cp = Cq + (size_t) col * ldc;
        double c[RR];
#pragma unroll
        for (int k = 0; k < RR; ++k) {
            const int i = lane + 64 * k;
            c[k] = i < m ? cp[i] : 0.0;
        }
        for (int jj = 0; jj < n; ++jj) {
            const int j = tr ? jj : n - 1 - jj;
            const double tj = ts[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            qb_regs_reflect<RR>(Vs + j * ld, j, m, tj, c, lane);
        }
#pragma unroll
        for (int k = 0; k < RR; ++k) {
            const int i = lane + 64 * k;
            if (i < m) cp[i] = c[k];
        }
    }
}

// Q(i, c) = (i == c), m x n per matrix
__global__ void __launch_bounds__(256) b_eye_kernel(double* __restrict__ Q, int m, int n, int ldq, size_t strideQ)
{
    double* Qq = Q + (size_t) blockIdx.x * strideQ;
    for (int idx = threadIdx.x; idx < m * n; idx += 256) {
        const int c = idx / m, i = idx - c * m;
        Qq[(size_t) c * ldq + i] = i == c ? 1.0 : 0.0;
    }
}

// info[q] = 0 or the smallest i + 1 with R(i, i) == 0; info == 0: rows 0 .. n-1 of B <- R^-1 of them.  LDS: Rs[c * (n + 1) + r], a word.
__host__ __device__ __forceinline__ size_t b_trsm_lds(int n) { return sizeof(double) * ((size_t) n * (n + 1) + 2); }

__global__ void __launch_bounds__(256) b_trsm_kernel(const double* __restrict__ A, int n, int lda, size_t strideA, double* __restrict__ B,
                                                     int nrhs, int ldb, size_t strideB, int* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lr = n + 1;
    const size_t q = blockIdx.x;
    double* Rs = sm;
    int* sinfo = (int*) (Rs + (size_t) n * lr);
    const double* Aq = A + q * strideA;
    double* Bq = B + q * strideB;
    for (int idx = t; idx < n * n; idx += 256) {
        const int c = idx / n, r = idx - c * n;
        Rs[c * lr + r] = r <= c ? Aq[(size_t) c * lda + r] : 0.0;
    }
    __syncthreads();
    if (t == 0) info[q] = *sinfo = qb_info_serial(Rs, lr, n);
    __syncthreads();
    if (*sinfo) return;
    for (int r = t; r < nrhs; r += 256) qb_trsv(Rs, lr, n, Bq + (size_t) r * ldb);    // (a thread owns its column of B: no other thread touches it)
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Section 8b: column pivoting.  bp_wave_kernel<W> and bp_wg_kernel are the pivoted siblings of the two factorisation kernels above
// (LAPACK dlaqp2 per matrix: every column free, the partial norms downdated and recomputed by its rule); with nrhs > 0 they carry the
// right-hand sides along and end with the rank-revealing solve (bp_tz_sweep, bp_solve_cols).  bp_solve_kernel is that solve on its
// own (the composed route), bp_rank_kernel the rank from the diagonal.  The Householder step itself is the unpivoted kernels' (qb_wave_col,
// qb_wg_col): a pivoted kernel adds the pivot search and the swap before it and the downdate of the norms after it, so on columns
// that are already in pivot order its factors and tau are bitwise qrd_b_geqrf's.
//
// The norm state of column c (vn1: the running partial norm, vn2: its value when last computed exactly) and jpvt[c] live in lane c of
// the wave (wave 0 of the workgroup route): n <= 64.  Every arg-max, swap and sum runs in an order that (m, n, nrhs) fix.
// ---------------------------------------------------------------------------------------------------------------------------------
#define BP_TOL3Z 1.4901161193847656e-08          // sqrt(DBL_EPSILON), dlaqp2's tol3z

// the index of the largest v over the wave, the lowest index on a tie; lanes that do not compete pass v < 0.  A butterfly on (v, idx)
// pairs under a total order: the same pair in every lane, whatever the data.  (NaN breaks the order: the callers clamp the result.)
__device__ __forceinline__ int bp_wave_argmax(double v, int idx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    return __builtin_amdgcn_readfirstlane(idx);
}

// dlaqp2's downdate of one column after step j: a = A(j, c).  Returns true where the norm has to be recomputed from rows j+1 .. m-1.
__device__ __forceinline__ bool bp_downdate(double a, double& vn1, double vn2)
{
    if (vn1 == 0.0) return false;
    const double tq = fabs(a) / vn1;
    const double temp = fmax(0.0, 1.0 - tq * tq);
    const double rr = vn1 / vn2;
    if (temp * (rr * rr) <= BP_TOL3Z) return true;
    vn1 *= sqrt(temp);
    return false;
}

// the length of the leading run of |R(i,i)| > rcond |R(0,0)|; d: R(lane, lane) in lanes < n (n <= 64)
__device__ __forceinline__ int bp_wave_rank(double d, int n, int lane, double rcond)
{
    const double thr = rcond * fabs(__shfl(d, 0));
    const unsigned long long small = __ballot(lane < n && !(fabs(d) > thr));
    return small ? __ffsll((long long) small) - 1 : n;
}

// One wave.  The trapezoid [R11 R12] (r x n, Rs[c * ldr + i] = R(i, c)) -> [T11 0] Z by r reflectors from the right (LAPACK dlatrz):
// i = r-1 .. 0: dlarfg on [T(i,i), R(i, r .. n-1)], applied to rows 0 .. i-1.  Reflector i stays in R(i, r .. n-1), its tau in
// Rs[1 + i] (below the diagonal of column 0, which nothing here reads).  0 < r < n <= 64.
__device__ __forceinline__ void bp_tz_sweep(double* Rs, int ldr, int n, int r, int lane)
{
    const int l = n - r;
    for (int i = r - 1; i >= 0; --i) {
        const double x = lane < l ? Rs[(r + lane) * ldr + i] : 0.0;
        const double ssq = qb_wave_sum(x * x);
        const double alpha = Rs[i * ldr + i];
        double ti = 0.0;
        if (ssq != 0.0) {                     // (the same value in every lane)
            double beta, scal;
            ti = qb_larfg(alpha, ssq, beta, scal);
            QB_WAVE_SYNC();                   // (every lane has read alpha and its x)
            if (lane < l) Rs[(r + lane) * ldr + i] = x * scal;
            if (lane == 0) Rs[i * ldr + i] = beta;
            QB_WAVE_SYNC();
            if (lane < i) {                   // lane k: row k, w = T(k,i) + R(k, r..) . v
                double w = Rs[i * ldr + lane];
                for (int c = 0; c < l; ++c) w = fma(Rs[(r + c) * ldr + lane], Rs[(r + c) * ldr + i], w);
                const double tw = ti * w;
                Rs[i * ldr + lane] -= tw;
                for (int c = 0; c < l; ++c) Rs[(r + c) * ldr + lane] = fma(-tw, Rs[(r + c) * ldr + i], Rs[(r + c) * ldr + lane]);
            }
            QB_WAVE_SYNC();
        }
        if (lane == 0) Rs[1 + i] = ti;
    }
    QB_WAVE_SYNC();
}

// One wave, lane k < nrhs <= 64: column k of Xs (Xs[k * ldx + i], rows 0 .. n-1 of Q^T b) <- T11^-1 of its first r rows, zeros below,
// and with cod != 0 Z^T of that (reflectors 0 .. r-1 in that order).  cod == 0 or r == n: the plain back substitution.
__device__ __forceinline__ void bp_solve_cols(const double* Rs, int ldr, double* Xs, int ldx, int n, int r, int nrhs, int cod, int lane)
{
    if (lane < nrhs) {
        double* xr = Xs + (size_t) lane * ldx;
        qb_trsv(Rs, ldr, r, xr);
        for (int k = r; k < n; ++k) xr[k] = 0.0;
        if (cod) {
            for (int i = 0; i < r; ++i) {
                const double ti = Rs[1 + i];
                if (ti == 0.0) continue;
                double w = xr[i];
                for (int c = r; c < n; ++c) w = fma(Rs[c * ldr + i], xr[c], w);
                const double tw = ti * w;
                xr[i] -= tw;
                for (int c = r; c < n; ++c) xr[c] = fma(-tw, Rs[c * ldr + i], xr[c]);
            }
        }
    }
    QB_WAVE_SYNC();
}

// Step J of the wave route and, while columns remain, the steps after it.  The steps are a compile-time recursion, not a loop: every
// index into the register file a[] is a constant, and each inner loop has constant bounds (a loop over j of this size is past what
// `#pragma unroll` will take, and a[] would then live in scratch memory).
template <int W, int J>
__device__ __forceinline__ void bp_wave_step(double (&a)[W], int n, int ntot, int lane, double& vn1, double& vn2, int& jp, double& tauv,
                                             double& diag)
{
    if constexpr (J < W) {
        constexpr int j = J;
        if (j >= n) return;                   // (wave-uniform)
        int p = bp_wave_argmax((lane >= j && lane < n) ? vn1 : -1.0, lane);
        if (p < j || p >= n) p = j;
        if (p != j) {                         // (wave-uniform: the swap is a select over the register file)
            const double aj = a[j];
            double ap = aj;
#pragma unroll
            for (int c = j + 1; c < W; ++c) {
                const double ac = a[c];
                ap = c == p ? ac : ap;
                a[c] = c == p ? aj : ac;
            }
            a[j] = ap;
            const int jpp = __builtin_amdgcn_readlane(jp, p), jpj = __builtin_amdgcn_readlane(jp, j);
            const double v1 = qb_bcast(vn1, j), v2 = qb_bcast(vn2, j);
            if (lane == j) jp = jpp;
            if (lane == p) { jp = jpj; vn1 = v1; vn2 = v2; }
        }
        qb_wave_col<W>(a, j, ntot, lane, tauv, diag);
        // lane c > j: downdate with A(j, c), which lane j holds
        double ajc = 0.0;
#pragma unroll
        for (int c = j + 1; c < W; ++c) {
            if (c < n) {
                const double v = qb_bcast(a[c], j);
                if (lane == c) ajc = v;
            }
        }
        const bool redo = lane > j && lane < n && bp_downdate(ajc, vn1, vn2);
        unsigned long long mask = __ballot(redo);
        while (mask) {                        // (rare; index order) the exact norm of rows j+1 .. of a column that tripped the safeguard
            const int c = __ffsll((long long) mask) - 1;
            mask &= mask - 1;
            double y = 0.0;
#pragma unroll
            for (int k = j + 1; k < W; ++k) y = k == c ? a[k] : y;
            y = lane > j ? y : 0.0;
            const double s = sqrt(qb_wave_sum(y * y));
            if (lane == c) vn1 = vn2 = s;
        }
        bp_wave_step<W, J + 1>(a, n, ntot, lane, vn1, vn2, jp, tauv, diag);
    }
}

// wave route.  Dynamic LDS as b_wave_kernel: the fused solve's staging only.
template <int W>
__global__ void __launch_bounds__(256) bp_wave_kernel(double* __restrict__ A, int m, int n, int lda, size_t strideA, int* __restrict__ jpvt,
                                                      size_t stridej, double* __restrict__ tau, size_t stridetau, double* __restrict__ B,
                                                      int nrhs, int ldb, size_t strideB, double rcond, int minnorm,
                                                      double* __restrict__ resid, int* __restrict__ rank, int batch)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;          // (no workgroup barrier below)
    double* Aq = A + q * strideA;
    double* Bq = nrhs ? B + q * strideB : nullptr;
    const int ntot = n + nrhs;
    const bool row = lane < m;
    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (row && c < n) v = Aq[(size_t) c * lda + lane];
        else if (row && c < ntot) v = Bq[(size_t) (c - n) * ldb + lane];
        a[c] = v;
    }
    double vn1 = 0.0, vn2 = 0.0;              // lane c < n: the norm state of column c
    int jp = lane;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            const double s = sqrt(qb_wave_sum(a[c] * a[c]));
            if (lane == c) vn1 = vn2 = s;
        }
    }
    double tauv = 0.0, diag = 0.0;            // lane j: tau[j] and R(j, j)
    bp_wave_step<W, 0>(a, n, ntot, lane, vn1, vn2, jp, tauv, diag);
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (row && c < n) Aq[(size_t) c * lda + lane] = a[c];
    if (lane < n) {
        tau[q * stridetau + lane] = tauv;
        jpvt[q * stridej + lane] = jp;
    }
    if (!nrhs) return;
    const int r = bp_wave_rank(diag, n, lane, rcond);
    if (rank && lane == 0) rank[q] = r;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c >= n && c < ntot) {
            const double y = lane >= r ? a[c] : 0.0;
            const double s = sqrt(qb_wave_sum(y * y));
            if (resid && lane == 0) resid[q * nrhs + (c - n)] = s;
        }
    }
    // staging as in b_wave_kernel: rows 0 .. n-1 of R and of Q^T B into this wave's LDS, the rest of Q^T B straight back
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;       // Rs[c * LW + i] = R(i, c)
    double* Xs = Rs + W * LW;                          // Xs[k * LW + i] = (Q^T B)(i, k), then X in pivoted order
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n) {
            if (lane < n) Rs[c * LW + lane] = a[c];
        } else if (c < ntot) {
            if (lane < n) Xs[(c - n) * LW + lane] = a[c];
            else if (row) Bq[(size_t) (c - n) * ldb + lane] = a[c];
        }
    }
    QB_WAVE_SYNC();
    const int cod = minnorm && r > 0 && r < n;
    if (cod) bp_tz_sweep(Rs, LW, n, r, lane);
    bp_solve_cols(Rs, LW, Xs, LW, n, r, nrhs, cod, lane);
    for (int k = 0; k < nrhs; ++k)
        if (lane < n) Bq[(size_t) k * ldb + jp] = Xs[k * LW + lane];
}

// workgroup route.  LDS: the image As of [A | B] as b_wg_kernel, red[4], two words (the pivot, the rank), 3 spare, nrm[64] (the
// initial norms on their way to wave 0's lanes): ntot * ld + QB_WG_SMALL doubles, what qrd_b_fits budgets.
__host__ __device__ __forceinline__ size_t bp_wg_lds(int m, int ntot) { return sizeof(double) * ((size_t) ntot * qb_ld(m) + QB_WG_SMALL); }

__global__ void __launch_bounds__(256) bp_wg_kernel(double* __restrict__ A, int m, int n, int lda, size_t strideA, int* __restrict__ jpvt,
                                                    size_t stridej, double* __restrict__ tau, size_t stridetau, double* __restrict__ B, int nrhs,
                                                    int ldb, size_t strideB, double rcond, int minnorm, double* __restrict__ resid,
                                                    int* __restrict__ rank)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = qb_ld(m), ntot = n + nrhs;
    double* As = sm;
    double* red = As + (size_t) ntot * ld;
    int* sw = (int*) (red + 4);               // sw[0]: the pivot of the step, sw[1]: the rank
    double* nrm = red + 8;
    double* Aq = A + q * strideA;
    double* Bq = nrhs ? B + q * strideB : nullptr;
    double* tq = tau + q * stridetau;
    for (int c = wv; c < ntot; c += 4) {
        const double* src = c < n ? Aq + (size_t) c * lda : Bq + (size_t) (c - n) * ldb;
        for (int i = lane; i < m; i += 64) As[c * ld + i] = src[i];
    }
    __syncthreads();
    for (int c = wv; c < n; c += 4) {         // the initial norms: one pass over the image
        double s = 0.0;
        for (int i = lane; i < m; i += 64) s = fma(As[c * ld + i], As[c * ld + i], s);
        s = qb_wave_sum(s);
        if (lane == 0) nrm[c] = sqrt(s);
    }
    __syncthreads();
    double vn1 = 0.0, vn2 = 0.0;              // wave 0, lane c < n: the norm state of column c
    int jp = lane;
    if (wv == 0 && lane < n) vn1 = vn2 = nrm[lane];
    for (int j = 0; j < n; ++j) {
        if (wv == 0) {
            int p = bp_wave_argmax((lane >= j && lane < n) ? vn1 : -1.0, lane);
            if (p < j || p >= n) p = j;
            if (lane == 0) sw[0] = p;
            if (p != j) {
                const int jpp = __builtin_amdgcn_readlane(jp, p), jpj = __builtin_amdgcn_readlane(jp, j);
                const double v1 = qb_bcast(vn1, j), v2 = qb_bcast(vn2, j);
                if (lane == j) jp = jpp;
                if (lane == p) { jp = jpj; vn1 = v1; vn2 = v2; }
            }
        }
        __syncthreads();
        const int p = sw[0];
        if (p != j) {                         // (the same value in every thread)
            double* vj = As + j * ld;
            double* vp = As + p * ld;
            for (int i = t; i < m; i += 256) {
                const double tmp = vj[i];
                vj[i] = vp[i];
                vp[i] = tmp;
            }
            __syncthreads();
        }
        const double tj = qb_wg_col(As, ld, m, j, ntot, red, t);
        if (t == 0) tq[j] = tj;
        __syncthreads();
        // wave 0 alone, while the others wait at the next step's barrier: lane c > j downdates with A(j, c); the columns that trip the
        // safeguard are recomputed from rows j+1 .. m-1 in index order
        if (wv == 0) {
            const bool live = lane > j && lane < n;
            const bool redo = live && bp_downdate(As[(live ? lane : 0) * ld + j], vn1, vn2);
            unsigned long long mask = __ballot(redo);
            while (mask) {
                const int c = __ffsll((long long) mask) - 1;
                mask &= mask - 1;
                double y = 0.0;
                for (int i = j + 1 + lane; i < m; i += 64) y = fma(As[c * ld + i], As[c * ld + i], y);
                y = sqrt(qb_wave_sum(y));
                if (lane == c) vn1 = vn2 = y;
            }
        }
    }
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < m; i += 64) Aq[(size_t) c * lda + i] = As[c * ld + i];
    if (wv == 0 && lane < n) jpvt[q * stridej + lane] = jp;
    if (!nrhs) return;
    if (wv == 0) {
        const int r0 = bp_wave_rank(lane < n ? As[lane * ld + lane] : 0.0, n, lane, rcond);
        if (lane == 0) {
            sw[1] = r0;
            if (rank) rank[q] = r0;
        }
    }
    __syncthreads();                          // (the factors have left the image: the solve may overwrite them)
    const int r = sw[1];
    if (resid)
        for (int c = n + wv; c < ntot; c += 4) {
            double y = 0.0;
            for (int i = r + lane; i < m; i += 64) y = fma(As[c * ld + i], As[c * ld + i], y);
            y = sqrt(qb_wave_sum(y));
            if (lane == 0) resid[q * nrhs + (c - n)] = y;
        }
    __syncthreads();
    if (wv == 0) {                            // (nrhs < 64: one lane per right-hand side)
        const int cod = minnorm && r > 0 && r < n;
        if (cod) bp_tz_sweep(As, ld, n, r, lane);
        bp_solve_cols(As, ld, As + (size_t) n * ld, ld, n, r, nrhs, cod, lane);
    }
    __syncthreads();
    for (int c = n + wv; c < ntot; c += 4)
        for (int i = n + lane; i < m; i += 64) Bq[(size_t) (c - n) * ldb + i] = As[c * ld + i];
    if (wv == 0 && lane < n)
        for (int k = 0; k < nrhs; ++k) Bq[(size_t) k * ldb + jp] = As[(n + k) * ld + lane];
}

// The solve of the composed route, one wave per (matrix, 64 right-hand sides): B holds Q^T B.  LDS: Rs[c * (n + 1) + i] (the triangle,
// zeros below it), Xs[k * (n + 1) + i] for 64 columns.
__host__ __device__ __forceinline__ size_t bp_solve_lds(int n) { return sizeof(double) * ((size_t) (n + 64) * (n + 1)); }

__global__ void __launch_bounds__(64) bp_solve_kernel(const double* __restrict__ A, int m, int n, int lda, size_t strideA,
                                                      const int* __restrict__ jpvt, size_t stridej, double* __restrict__ B, int nrhs, int ldb,
                                                      size_t strideB, double rcond, int minnorm, double* __restrict__ resid,
                                                      int* __restrict__ rank)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x, lr = n + 1;
    const size_t q = blockIdx.x;
    double* Rs = sm;
    double* Xs = Rs + (size_t) n * lr;
    const double* Aq = A + q * strideA;
    double* Bq = B + q * strideB;
    for (int idx = lane; idx < n * n; idx += 64) {
        const int c = idx / n, i = idx - c * n;
        Rs[c * lr + i] = i <= c ? Aq[(size_t) c * lda + i] : 0.0;
    }
    int jp = lane < n ? jpvt[q * stridej + lane] : 0;
    if (jp < 0 || jp >= n) jp = lane < n ? lane : 0;          // (a jpvt that is none of geqp3's must not carry a store out of the block)
    QB_WAVE_SYNC();
    const int r = bp_wave_rank(lane < n ? Rs[lane * lr + lane] : 0.0, n, lane, rcond);
    if (rank && blockIdx.y == 0 && lane == 0) rank[q] = r;
    const int cod = minnorm && r > 0 && r < n;
    if (cod) bp_tz_sweep(Rs, lr, n, r, lane);
    for (int k0 = (int) blockIdx.y * 64; k0 < nrhs; k0 += (int) gridDim.y * 64) {
        const int nk = nrhs - k0 < 64 ? nrhs - k0 : 64;
        for (int k = 0; k < nk; ++k) {
            const double* col = Bq + (size_t) (k0 + k) * ldb;
            double y = 0.0;
            for (int i = r + lane; i < m; i += 64) y = fma(col[i], col[i], y);
            y = sqrt(qb_wave_sum(y));
            if (resid && lane == 0) resid[q * nrhs + (k0 + k)] = y;
            if (lane < n) Xs[k * lr + lane] = col[lane];
        }
        QB_WAVE_SYNC();
        bp_solve_cols(Rs, lr, Xs, lr, n, r, nk, cod, lane);
        for (int k = 0; k < nk; ++k)
            if (lane < n) Bq[(size_t) (k0 + k) * ldb + jp] = Xs[k * lr + lane];
        QB_WAVE_SYNC();                       // (Xs is read no more)
    }
}

// rank[q] from the diagonal of R, one thread per matrix
__global__ void __launch_bounds__(256) bp_rank_kernel(const double* __restrict__ A, int n, int lda, size_t strideA, double rcond,
                                                      int* __restrict__ rank, int batch)
{
    const size_t q = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t) batch) return;
    const double* Aq = A + q * strideA;
    const double thr = rcond * fabs(Aq[0]);
    int r = 0;
    while (r < n && fabs(Aq[(size_t) r * lda + r]) > thr) ++r;
    rank[q] = r;
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int b_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(b_wg_kernel),       reinterpret_cast<const void*>(b_ormqr_kernel<1>),
                               reinterpret_cast<const void*>(b_ormqr_kernel<2>), reinterpret_cast<const void*>(b_ormqr_kernel<4>),
                               reinterpret_cast<const void*>(b_ormqr_kernel<8>), reinterpret_cast<const void*>(b_wave_kernel<32>),
                               reinterpret_cast<const void*>(bp_wg_kernel),      reinterpret_cast<const void*>(bp_wave_kernel<32>),
                               reinterpret_cast<const void*>(bp_solve_kernel)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

template <int W>
static void b_launch_wave(hipStream_t s, double* A, int m, int n, int lda, size_t sa, double* tau, size_t st, double* B, int nrhs, int ldb,
                          size_t sb, int* info, int batch)
{
    const size_t lds = nrhs ? sizeof(double) * 4 * 2 * W * (W + 1) : 0;
    hipLaunchKernelGGL(b_wave_kernel<W>, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), lds, s, A, m, n, lda, sa, tau, st, B, nrhs, ldb,
                       sb, info, batch);
}

template <int W>
static void bp_launch_wave(hipStream_t s, double* A, int m, int n, int lda, size_t sa, int* jpvt, size_t sj, double* tau, size_t st, double* B,
                           int nrhs, int ldb, size_t sb, double rcond, int minnorm, double* resid, int* rank, int batch)
{
    const size_t lds = nrhs ? sizeof(double) * 4 * 2 * W * (W + 1) : 0;
    hipLaunchKernelGGL(bp_wave_kernel<W>, dim3((unsigned) (((size_t) batch + 3) / 4)), dim3(256), lds, s, A, m, n, lda, sa, jpvt, sj, tau, st, B,
                       nrhs, ldb, sb, rcond, minnorm, resid, rank, batch);
}

extern "C" {

int qrd_b_max_rows(int ncols)
{
    if (ncols < 1 || ncols > QRD_B_MAX_N) return 0;
    // rows that fit for EVERY column count of the class: 32 * 514 and 64 * 258 doubles, plus the small arrays, within 160 KiB
    return ncols <= 32 ? QRD_B_MAX_ROWS : QRD_B_MAX_ROWS / 2;
}

// what the kernels hold: at most QRD_B_MAX_ROWS rows (b_ormqr_kernel's registers) and ncols columns at qb_ld(m) plus the small arrays
// (QB_WG_SMALL doubles cover b_wg_kernel and b_ormqr_kernel too) within QB_LDS_CAP.  Every shape within qrd_b_max_rows fits.
int qrd_b_fits(int m, int ncols)
{
    return ncols >= 1 && ncols <= QRD_B_MAX_N && m >= 1 && m <= QRD_B_MAX_ROWS &&
           sizeof(double) * ((size_t) ncols * qb_ld(m) + QB_WG_SMALL) <= QB_LDS_CAP;
}

int qrd_b_wave_route(int m, int ncols) { return m <= 64 && ncols <= 32; }

// [A | B] factored over the first n columns; nrhs > 0: B's columns ride along (B <- Q^T B), then info and, where it is 0, R X = B in the
// same launch.  -7: shape not taken
int qrd_b_geqrf(void* stream, double* A, int m, int n, int lda, size_t strideA, double* tau, size_t stridetau, double* B, int nrhs, int ldb,
                size_t strideB, int* info, int batch)
{
    const int ntot = n + nrhs;
    if (batch <= 0) return 0;
    if (n < 1 || m < n || nrhs < 0 || !qrd_b_fits(m, ntot) || lda < m || (nrhs && (!B || ldb < m || !info)))
        return -7;
    const int rc = b_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_b_wave_route(m, ntot)) {
        if (ntot <= 8) b_launch_wave<8>(s, A, m, n, lda, strideA, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
        else if (ntot <= 16) b_launch_wave<16>(s, A, m, n, lda, strideA, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
        else b_launch_wave<32>(s, A, m, n, lda, strideA, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
    } else {
        hipLaunchKernelGGL(b_wg_kernel, dim3((unsigned) batch), dim3(256), b_wg_lds(m, ntot), s, A, m, n, lda, strideA, tau, stridetau, B, nrhs,
                           ldb, strideB, info);
    }
    return (int) hipGetLastError();
}

int qrd_b_ormqr(void* stream, int trans_t, const double* A, int m, int n, int lda, size_t strideA, const double* tau, size_t stridetau,
                double* Cm, int nrhs, int ldc, size_t strideC, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || !qrd_b_fits(m, n) || lda < m || ldc < m || nrhs < 1) return -7;
    const int rc = b_allow_lds();
    if (rc) return rc;
    int gy = (nrhs + 15) / 16;                // four columns per wave; beyond 1024 workgroups per matrix the waves loop
    if (gy > 1024) gy = 1024;
    const dim3 grid((unsigned) batch, (unsigned) gy);
    const size_t lds = b_ormqr_lds(m, n);
    hipStream_t s = (hipStream_t) stream;
#define B_ORMQR(RR) hipLaunchKernelGGL(b_ormqr_kernel<RR>, grid, dim3(256), lds, s, trans_t, A, m, n, lda, strideA, tau, stridetau, Cm, nrhs, ldc, strideC)
    if (m <= 64) B_ORMQR(1);
    else if (m <= 128) B_ORMQR(2);
    else if (m <= 256) B_ORMQR(4);
    else B_ORMQR(8);
#undef B_ORMQR
    return (int) hipGetLastError();
}

int qrd_b_eye(void* stream, double* Q, int m, int n, int ldq, size_t strideQ, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || ldq < m) return -7;
    hipLaunchKernelGGL(b_eye_kernel, dim3((unsigned) batch), dim3(256), 0, (hipStream_t) stream, Q, m, n, ldq, strideQ);
    return (int) hipGetLastError();
}

int qrd_b_trsm(void* stream, const double* A, int n, int lda, size_t strideA, double* B, int nrhs, int ldb, size_t strideB, int* info, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || lda < n || ldb < n || nrhs < 1 || !info) return -7;
    hipLaunchKernelGGL(b_trsm_kernel, dim3((unsigned) batch), dim3(256), b_trsm_lds(n), (hipStream_t) stream, A, n, lda, strideA, B, nrhs, ldb,
                       strideB, info);
    return (int) hipGetLastError();
}

// [A | B] factored with column pivoting over the first n columns (dlaqp2 per matrix; jpvt 0-based).  nrhs > 0 (the fused gelsp / gelsy):
// B's columns ride along, then the rank r from the diagonal (|R(i,i)| > rcond |R(0,0)|, rcond >= 0), resid (may be NULL), rank (may be
// NULL) and X in the caller's column order (minnorm: through the complete orthogonal decomposition), all in the one launch.
int qrd_b_geqp3(void* stream, double* A, int m, int n, int lda, size_t strideA, int* jpvt, size_t stridej, double* tau, size_t stridetau,
                double* B, int nrhs, int ldb, size_t strideB, double rcond, int minnorm, double* resid, int* rank, int batch)
{
    const int ntot = n + nrhs;
    if (batch <= 0) return 0;
    if (n < 1 || m < n || nrhs < 0 || !qrd_b_fits(m, ntot) || lda < m || !jpvt || (nrhs && (!B || ldb < m))) return -7;
    const int rc = b_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_b_wave_route(m, ntot)) {
#define BP_WAVE(W) bp_launch_wave<W>(s, A, m, n, lda, strideA, jpvt, stridej, tau, stridetau, B, nrhs, ldb, strideB, rcond, minnorm, resid, rank, batch)
        if (ntot <= 4) BP_WAVE(4);
        else if (ntot <= 8) BP_WAVE(8);
        else if (ntot <= 16) BP_WAVE(16);
        else BP_WAVE(32);
#undef BP_WAVE
    } else {
        hipLaunchKernelGGL(bp_wg_kernel, dim3((unsigned) batch), dim3(256), bp_wg_lds(m, ntot), s, A, m, n, lda, strideA, jpvt, stridej, tau,
                           stridetau, B, nrhs, ldb, strideB, rcond, minnorm, resid, rank);
    }
    return (int) hipGetLastError();
}

int qrd_b_rank(void* stream, const double* A, int n, int lda, size_t strideA, double rcond, int* rank, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || lda < n || !rank) return -7;
    hipLaunchKernelGGL(bp_rank_kernel, dim3((unsigned) (((size_t) batch + 255) / 256)), dim3(256), 0, (hipStream_t) stream, A, n, lda, strideA,
                       rcond, rank, batch);
    return (int) hipGetLastError();
}

// the solve of the composed route: B holds Q^T B (m rows), A the factors of qrd_b_geqp3; rank, resid and X as there
int qrd_b_solve_piv(void* stream, const double* A, int m, int n, int lda, size_t strideA, const int* jpvt, size_t stridej, double* B, int nrhs,
                    int ldb, size_t strideB, double rcond, int minnorm, double* resid, int* rank, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || n > QRD_B_MAX_N || m < n || lda < n || ldb < m || nrhs < 1 || !jpvt) return -7;
    const int rc = b_allow_lds();
    if (rc) return rc;
    int gy = (nrhs + 63) / 64;                // 64 columns per wave; beyond 1024 workgroups per matrix the waves loop
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(bp_solve_kernel, dim3((unsigned) batch, (unsigned) gy), dim3(64), bp_solve_lds(n), (hipStream_t) stream, A, m, n, lda,
                       strideA, jpvt, stridej, B, nrhs, ldb, strideB, rcond, minnorm, resid, rank);
    return (int) hipGetLastError();
}

}   // extern "C"
