// qr_batched_minnorm.hip -- kernels of the batched minimum-norm solves (qr_batched_minnorm.c, mi355x_qr.h section 8e): with F = Q R
// (rows x cols, rows >= cols, full rank) the minimum-norm solution of F^T X = B is X = Q [R^-T B ; 0], per member of a batch.
//
//   bm_wave_kernel<W, TR>  rows <= 64, cols + nrhs <= W <= 32: one wave per member, four members per workgroup.  Lane i holds row i of F
//                      in W registers; the factorisation is b_wave_kernel's (qr_batched.hip) column step, qb_wave_col, the right-hand
//                      sides untouched by it; then R^T y = b on an LDS image of R, one lane per right-hand side, and the reflectors
//                      cols-1 .. 0 on [y ; 0] with the column back in registers, one butterfly each
//   bm_wg_kernel       everything else that holds cols + nrhs columns in LDS: one workgroup per member, [F | X] resident at
//                      ld = qb_ld(rows); b_wg_kernel's column step, qb_wg_col; then the same two stages, wave w on right-hand sides
//                      w, w + 4, ..
//   bm_apply_kernel<RR> the solve on factors that exist (any nrhs): grid (batch, groups of 16 right-hand sides), whole columns of the factors
//                      in LDS, one wave per right-hand side with the column in registers
//   bm_transpose_kernel D (cols x rows) = S^T per member through a 32 x 33 LDS tile: reads and writes along contiguous addresses
//
// TR (bm_wave_kernel) / tr (bm_wg_kernel): the member is given as the wide matrix A = F^T (cols x rows, column-major), read through the
// transposed index map, F (A, lda) -> (A^T); the factors then go to a buffer of their own.  Otherwise F is factored in place.
//
// The two factorisation loops call the column steps that b_wave_kernel and b_wg_kernel call (qr_batched_dev.h), with the end of the
// update at `cols` where those pass cols + nrhs: the factors and tau are bitwise those of qrd_b_geqrf on the same route.  The callers
// add the transposed load, the copy of tau kept in LDS and the solve.  Every sum runs in an order that (rows, cols, nrhs) fix; no atomics.
//
// info: 0, or i + 1 for the smallest i with R(i,i) == 0 exactly; such a member's right-hand sides are not written at all.
#include "qr_batched_dev.h"

#define BM_MAXN QRD_B_MAX_N
#define BM_COLS 16                        // right-hand sides per workgroup of bm_apply_kernel: four per wave

static_assert(QRD_B_MAX_N == 64, "the forward substitution of bm_apply_kernel holds one row of R^T y = b per lane");

// ---------------------------------------------------------------------------------------------------------------------------------
// wave route.  Dynamic LDS per wave: Rs (W x (W + 1), Rs[c * LW + r] = R(r, c)) and Xs (W x (W + 1), Xs[k * LW + r] = b_k(r), then y).
// A and F are the same array for the in-place call: neither is __restrict__.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W, bool TR>
__global__ void __launch_bounds__(256) bm_wave_kernel(const double* A, int m, int n, int lda, size_t strideA, double* F, int ldf, size_t strideF,
                                                      double* __restrict__ tau, size_t stridetau, double* __restrict__ B, int nrhs, int ldb,
                                                      size_t strideB, int* __restrict__ info, int batch)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t) blockIdx.x * 4 + wv;
    if (q >= (size_t) batch) return;          // (no workgroup barrier below: the waves of a workgroup are independent)
    const double* Aq = A + q * strideA;
    double* Fq = F + q * strideF;
    double* Bq = B + q * strideB;
    const int ntot = n + nrhs;
    const bool row = lane < m;
    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = 0.0;
        if (row && c < n) v = TR ? Aq[(size_t) lane * lda + c] : Aq[(size_t) c * lda + lane];   // TR: lane i reads column i of A, contiguous
        a[c] = v;
    }
    double tauv = 0.0, diag = 1.0;            // lane j: tau[j] and R(j, j)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) qb_wave_col<W>(a, j, n, lane, tauv, diag);         // (wave-uniform; the update ends at n: the right-hand sides are not in a[] yet)
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (row && c < n) Fq[(size_t) c * ldf + lane] = a[c];
    if (lane < n) tau[q * stridetau + lane] = tauv;
    const int inf = qb_info_wave(diag, n, lane);
    if (lane == 0) info[q] = inf;
    if (inf) return;                          // (all or nothing: B is as it was)
    // staging: R and rows 0 .. n-1 of B into this wave's LDS
    constexpr int LW = W + 1;
    double* Rs = sm + (size_t) wv * 2 * W * LW;
    double* Xs = Rs + W * LW;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c < n && lane < n) Rs[c * LW + lane] = a[c];
    for (int k = 0; k < nrhs; ++k)
        if (lane < n) Xs[k * LW + lane] = Bq[(size_t) k * ldb + lane];
    QB_WAVE_SYNC();
    if (lane < nrhs) qb_trsv_t(Rs, LW, n, Xs + lane * LW);    // (nrhs < W <= 32: one lane per right-hand side) R^T y = b
    QB_WAVE_SYNC();
    // [y ; 0] back into the registers beside F, then H_0 .. H_{n-1} applied last first: one butterfly per reflector and column
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c >= n && c < ntot) a[c] = lane < n ? Xs[(c - n) * LW + lane] : 0.0;
#pragma unroll
    for (int jj = 0; jj < W; ++jj) {
        const int j = W - 1 - jj;             // (a constant once unrolled, as every index into a[])
        if (j < n) {                          // (wave-uniform)
            const double tj = __shfl(tauv, j);
            if (tj != 0.0) {                  // (tau == 0: H = I; wave-uniform)
                const double v = lane > j ? a[j] : (lane == j ? 1.0 : 0.0);
#pragma unroll
                for (int c = j + 1; c < W; ++c) {
                    if (c >= n && c < ntot) {
                        const double tw = tj * qb_wave_sum(v * a[c]);
                        a[c] = fma(-tw, v, a[c]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (row && c >= n && c < ntot) Bq[(size_t) (c - n) * ldb + lane] = a[c];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: As[c * ld + i] = column c of [F | X], ld = qb_ld(m); then red[4], a word for info, 3 spare, ts[64] (tau):
// (n + nrhs) * ld + QB_WG_SMALL doubles, what qrd_b_fits budgets.
// ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ size_t bm_wg_lds(int m, int ntot) { return sizeof(double) * ((size_t) ntot * qb_ld(m) + QB_WG_SMALL); }

__global__ void __launch_bounds__(256) bm_wg_kernel(int tr, const double* A, int m, int n, int lda, size_t strideA, double* F, int ldf,
                                                    size_t strideF, double* __restrict__ tau, size_t stridetau, double* __restrict__ B, int nrhs,
                                                    int ldb, size_t strideB, int* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = qb_ld(m), ntot = n + nrhs;
    double* As = sm;
    double* red = As + (size_t) ntot * ld;
    int* sinfo = (int*) (red + 4);
    double* ts = red + 8;
    const double* Aq = A + q * strideA;
    double* Fq = F + q * strideF;
    double* Bq = B + q * strideB;
    double* tq = tau + q * stridetau;
    if (tr) {                                 // row i of F is column i of A: read along it, write the image transposed
        for (int i = wv; i < m; i += 4) {
            const double* src = Aq + (size_t) i * lda;
            for (int c = lane; c < n; c += 64) As[c * ld + i] = src[c];
        }
    } else {
        for (int c = wv; c < n; c += 4) {
            const double* src = Aq + (size_t) c * lda;
            for (int i = lane; i < m; i += 64) As[c * ld + i] = src[i];
        }
    }
    for (int c = n + wv; c < ntot; c += 4) {  // [b ; 0]
        const double* src = Bq + (size_t) (c - n) * ldb;
        for (int i = lane; i < m; i += 64) As[c * ld + i] = i < n ? src[i] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double tj = qb_wg_col(As, ld, m, j, n, red, t);         // (the update ends at n: the right-hand sides take no part)
        if (t == 0) { tq[j] = tj; ts[j] = tj; }
        __syncthreads();                      // (red and column j are read no more)
    }
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < m; i += 64) Fq[(size_t) c * ldf + i] = As[c * ld + i];
    if (t == 0) info[q] = *sinfo = qb_info_serial(As, ld, n);
    __syncthreads();
    if (*sinfo) return;                       // (all or nothing: B is as it was)
    if (t < nrhs) qb_trsv_t(As, ld, n, As + (size_t) (n + t) * ld);           // (nrhs < 64: one thread per right-hand side) R^T y = b
    __syncthreads();
    // wave wv: right-hand sides wv, wv + 4, ..: the reflectors n-1 .. 0 on [y ; 0], each a wave-strided dot product and a butterfly
    for (int c = n + wv; c < ntot; c += 4) {
        double* bc = As + c * ld;
        for (int j = n - 1; j >= 0; --j) {
            const double tj = ts[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            qb_col_reflect(As + j * ld, bc, j, m, tj, lane);
            QB_WAVE_SYNC();                   // (the next reflector reads the column under another lane map)
        }
        double* dst = Bq + (size_t) (c - n) * ldb;
        for (int i = lane; i < m; i += 64) dst[i] = bc[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// B <- Q [R^-T B(0:n) ; 0] from factors that exist.  LDS: Vs[c * ld + i] = column c of the factors (R on and above the diagonal, V
// below), then tau[n].  A wave takes a right-hand side.  Forward substitution, one lane per row (n <= 64): lane l holds b_l; for
// k = 0 .. n-1, y_k = b_k / R(k,k) goes to every lane and lane l > k does b_l <- fma(-R(k,l), y_k, b_l): row l's sum runs over k
// ascending.  Then the column is row lane + 64 r in register r (RR = 1, 2, 4 or 8, the smallest that holds m rows), rows >= n exact
// zeros, and the reflectors run n-1 .. 0 as in b_ormqr_kernel 'N'.  Every workgroup of a member evaluates info; the first writes it.
// ---------------------------------------------------------------------------------------------------------------------------------
#define BM_ROWREGS 8
static_assert(QRD_B_MAX_ROWS <= 64 * BM_ROWREGS, "a right-hand side is held in BM_ROWREGS registers per lane");

__host__ __device__ __forceinline__ size_t bm_apply_lds(int m, int n) { return sizeof(double) * ((size_t) n * qb_ld(m) + BM_MAXN); }

template <int RR>
__global__ void __launch_bounds__(256) bm_apply_kernel(const double* __restrict__ A, int m, int n, int lda, size_t strideA,
                                                       const double* __restrict__ tau, size_t stridetau, double* __restrict__ B, int nrhs,
                                                       int ldb, size_t strideB, int* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t q = blockIdx.x;
    const int ld = qb_ld(m);
    double* Vs = sm;
    double* ts = Vs + (size_t) n * ld;
    const double* Aq = A + q * strideA;
    double* Bq = B + q * strideB;
    for (int c = wv; c < n; c += 4)
        for (int i = lane; i < m; i += 64) Vs[c * ld + i] = Aq[(size_t) c * lda + i];
    if (t < n) ts[t] = tau[q * stridetau + t];
    __syncthreads();
    const int inf = qb_info_wave(lane < n ? Vs[lane * ld + lane] : 1.0, n, lane);    // (the same value in every wave of every workgroup of the member)
    if (blockIdx.y == 0 && t == 0) info[q] = inf;
    if (inf) return;
    for (int col = (int) blockIdx.y * 4 + wv; col < nrhs; col += (int) gridDim.y * 4) {       // (wave-uniform)
        double* cp = Bq + (size_t) col * ldb;
        double b = lane < n ? cp[lane] : 0.0;
        for (int k = 0; k < n; ++k) {
            const double yk = qb_bcast(b, k) / Vs[k * ld + k];
            if (lane == k) b = yk;
            else if (lane > k && lane < n) b = fma(-Vs[lane * ld + k], yk, b);
        }
        double c[RR];
        c[0] = b;                             // (lanes >= n hold zero)
#pragma unroll
        for (int r = 1; r < RR; ++r) c[r] = 0.0;
        for (int j = n - 1; j >= 0; --j) {
            const double tj = ts[j];
            if (tj == 0.0) continue;          // (H = I; wave-uniform)
            qb_regs_reflect<RR>(Vs + j * ld, j, m, tj, c, lane);
        }
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            const int i = lane + 64 * r;
            if (i < m) cp[i] = c[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// D (cols x rows, ldd) = S^T (S: rows x cols, lds) per member; blockIdx.y walks the 32 x 32 tiles.  tile[c][r] = S(r0 + r, c0 + c).
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bm_transpose_kernel(const double* __restrict__ S, int rows, int cols, int lds, size_t strideS,
                                                           double* __restrict__ D, int ldd, size_t strideD)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int tr = (rows + 31) / 32;
    const int r0 = ((int) blockIdx.y % tr) * 32, c0 = ((int) blockIdx.y / tr) * 32;
    const double* Sq = S + (size_t) blockIdx.x * strideS;
    double* Dq = D + (size_t) blockIdx.x * strideD;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = ty + 8 * k;
        if (r0 + tx < rows && c0 + c < cols) tile[c][tx] = Sq[(size_t) (c0 + c) * lds + r0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k;
        if (c0 + tx < cols && r0 + r < rows) Dq[(size_t) (r0 + r) * ldd + c0 + tx] = tile[tx][r];
    }
}

// the kernels that may ask for more than 64 KiB of LDS (qr_allow_lds)
static int bm_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(bm_wg_kernel),
                               reinterpret_cast<const void*>(bm_apply_kernel<1>),
                               reinterpret_cast<const void*>(bm_apply_kernel<2>),
                               reinterpret_cast<const void*>(bm_apply_kernel<4>),
                               reinterpret_cast<const void*>(bm_apply_kernel<8>),
                               reinterpret_cast<const void*>(bm_wave_kernel<32, false>),
                               reinterpret_cast<const void*>(bm_wave_kernel<32, true>)};
    return qr_allow_lds(fns, QB_LDS_CAP, done);
}

template <int W>
static void bm_launch_wave(hipStream_t s, int tr, const double* A, int m, int n, int lda, size_t sa, double* F, int ldf, size_t sf, double* tau,
                           size_t st, double* B, int nrhs, int ldb, size_t sb, int* info, int batch)
{
    const size_t lds = sizeof(double) * 4 * 2 * W * (W + 1);
    const dim3 grid((unsigned) (((size_t) batch + 3) / 4));
    if (tr)
        hipLaunchKernelGGL((bm_wave_kernel<W, true>), grid, dim3(256), lds, s, A, m, n, lda, sa, F, ldf, sf, tau, st, B, nrhs, ldb, sb, info, batch);
    else
        hipLaunchKernelGGL((bm_wave_kernel<W, false>), grid, dim3(256), lds, s, A, m, n, lda, sa, F, ldf, sf, tau, st, B, nrhs, ldb, sb, info, batch);
}

extern "C" {

// The fused factor + solve, one launch.  (m, n): the shape of the tall matrix F that is factored, m >= n, n + nrhs columns held
// (qrd_b_fits(m, n + nrhs)).  tr == 0: F is A (lda >= m); tr != 0: F is the transpose of A (n x m, lda >= n).  The factors go to
// F (ldf >= m; may be A itself when tr == 0), tau (n per member).  B: m x nrhs (ldb >= m), rows 0 .. n-1 hold the right-hand sides on
// entry, X on return where info is 0.  -7: shape not taken
int qrd_bm_fused(void* stream, int tr, const double* A, int m, int n, int lda, size_t strideA, double* F, int ldf, size_t strideF, double* tau,
                 size_t stridetau, double* B, int nrhs, int ldb, size_t strideB, int* info, int batch)
{
    const int ntot = n + nrhs;
    if (batch <= 0) return 0;
    if (n < 1 || m < n || nrhs < 1 || !qrd_b_fits(m, ntot) || lda < (tr ? n : m) || ldf < m || ldb < m || !A || !F || !tau || !B || !info)
        return -7;
    const int rc = bm_allow_lds();
    if (rc) return rc;
    hipStream_t s = (hipStream_t) stream;
    if (qrd_b_wave_route(m, ntot)) {
        if (ntot <= 8) bm_launch_wave<8>(s, tr, A, m, n, lda, strideA, F, ldf, strideF, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
        else if (ntot <= 16) bm_launch_wave<16>(s, tr, A, m, n, lda, strideA, F, ldf, strideF, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
        else bm_launch_wave<32>(s, tr, A, m, n, lda, strideA, F, ldf, strideF, tau, stridetau, B, nrhs, ldb, strideB, info, batch);
    } else {
        hipLaunchKernelGGL(bm_wg_kernel, dim3((unsigned) batch), dim3(256), bm_wg_lds(m, ntot), s, tr, A, m, n, lda, strideA, F, ldf, strideF, tau,
                           stridetau, B, nrhs, ldb, strideB, info);
    }
    return (int) hipGetLastError();
}

// B <- Q [R^-T B(0:n) ; 0] from the factors of qrd_b_geqrf / qrd_b_geqp3, any nrhs >= 1, info as above.  One launch.
int qrd_bm_apply(void* stream, const double* A, int m, int n, int lda, size_t strideA, const double* tau, size_t stridetau, double* B, int nrhs,
                 int ldb, size_t strideB, int* info, int batch)
{
    if (batch <= 0) return 0;
    if (n < 1 || m < n || !qrd_b_fits(m, n) || lda < m || ldb < m || nrhs < 1 || !A || !tau || !B || !info) return -7;
    const int rc = bm_allow_lds();
    if (rc) return rc;
    int gy = (nrhs + BM_COLS - 1) / BM_COLS;  // four columns per wave; beyond 1024 workgroups per member the waves loop
    if (gy > 1024) gy = 1024;
    const dim3 grid((unsigned) batch, (unsigned) gy);
    const size_t lds = bm_apply_lds(m, n);
    hipStream_t s = (hipStream_t) stream;
#define BM_APPLY(RR) hipLaunchKernelGGL(bm_apply_kernel<RR>, grid, dim3(256), lds, s, A, m, n, lda, strideA, tau, stridetau, B, nrhs, ldb, strideB, info)
    if (m <= 64) BM_APPLY(1);
    else if (m <= 128) BM_APPLY(2);
    else if (m <= 256) BM_APPLY(4);
    else BM_APPLY(8);
#undef BM_APPLY
    return (int) hipGetLastError();
}

// D_q (cols x rows, ldd >= cols) = S_q^T (S_q: rows x cols, lds >= rows), out of place
int qrd_bm_transpose(void* stream, const double* S, int rows, int cols, int lds, size_t strideS, double* D, int ldd, size_t strideD, int batch)
{
    if (batch <= 0) return 0;
    if (rows < 1 || cols < 1 || rows > QRD_B_MAX_ROWS || cols > QRD_B_MAX_ROWS || lds < rows || ldd < cols || !S || !D) return -7;
    const int tiles = ((rows + 31) / 32) * ((cols + 31) / 32);
    hipLaunchKernelGGL(bm_transpose_kernel, dim3((unsigned) batch, (unsigned) tiles), dim3(256), 0, (hipStream_t) stream, S, rows, cols, lds,
                       strideS, D, ldd, strideD);
    return (int) hipGetLastError();
}

}   // extern "C"
