// qr_svd.hip -- kernels of the one-sided block Jacobi SVD (qr_svd.c, mi355x_qr.h section 7).
//
//   jsvd_pair_kernel       one workgroup per block pair (p, q) of a tournament round: up to 64 columns of G (two blocks of 32)
//                            1. S = G_pq^T G_pq (64 x 64) on v_mfma_f64_16x16x4_f64, the rows streamed through LDS in chunks of 128
//                            2. the pair's measure max_{i<j} |s_ij| / sqrt(s_ii s_jj) into its slot; at or below tol the workgroup ends here
//                            3. cyclic Jacobi rotations (the smaller angle, |tan| <= 1) diagonalise S in LDS to the same threshold, their
//                               product J (64 x 64) is accumulated
//                            4. G_pq <- G_pq J, and V_pq <- V_pq J when rotations are accumulated, on MFMA tiles in chunks of 128 rows:
//                               every element is read once and written once (a matrix of at most 128 rows stays resident from step 1)
//   jsvd_fold_kernel       the slots of a sweep folded into its convergence word (a maximum: exact in any order)
//   jsvd_colnorm_kernel    column norms;  jsvd_gather_kernel: values by the sort permutation;  jsvd_permute_kernel: columns by it, in
//                          place along the permutation's cycles;  jsvd_normalise_kernel: columns / sigma, a zero column stays zero
//   jsvd_pinv_kernel       rows of Z^T c divided by the singular values above the threshold, zero for the others
//   jsvd_rt_kernel         R^T (lower triangular, zeros above) out of the factored matrix
//
// The self-pair (0, 0) of a matrix of at most 32 columns and a ragged last block are the same kernel: columns that do not exist are
// loaded as zero columns, never rotated (a zero column has s_ii = 0 and is skipped everywhere) and never stored.
//
// LDS images.  A chunk of 128 rows x 64 columns is kept column-major with a leading dimension of JS_LD = 130 doubles, S and J with
// JS_LS = 65.  8-byte accesses are served per 32-lane half, two banks per double: a half is conflict-free when its 32 double indices are
// distinct mod 32 (the reasoning at the top of qr_update.hip).  With the fragment maps of v_mfma_f64_16x16x4_f64 (A operand lane l =
// A[row l & 15][k l >> 4], B operand lane l = B[k l >> 4][col l & 15], C / D register r of lane l = D[row (l >> 4) + 4 r][col l & 15]):
//   Gram (both operands: lane & 15 along the columns, lane >> 4 along the rows): index = 130 (lane & 15) + (lane >> 4) + const =
//       2 (lane & 15) + {0, 1} (mod 32) -- 32 distinct values;
//   apply, chunk as the A operand (lane & 15 along the rows, lane >> 4 along the columns): k-step ks takes the columns
//       (ks & 7) + 8 (lane >> 4) + 32 (ks >> 3), so a half reads 16 rows of two columns 8 apart: index = (lane & 15) + {0, 8 * 130 = 16 (mod 32)}
//       -- 32 distinct values; J as the B operand of the same step reads 65 (lane & 15) + 8 (lane >> 4): two lanes per bank pair.
//
// Every sum runs in a fixed order (MFMA chains in row order, wave butterflies, waves in wave order) and every maximum is exact:
// repeated launches give bitwise-equal results.  No workgroup waits for another; no atomics.
#include <float.h>

#include "qr_common.h"
#include "qr_device.h"

#define JS_B QRD_JSVD_BLOCK
#define JS_W (2 * JS_B)
#define JS_CH 128
#define JS_LD (JS_CH + 2)
#define JS_LS (JS_W + 1)
#define JS_INNER_MAX 16                     /* inner sweeps over S per pair: quadratic convergence needs 5 to 8 from a full matrix */
#define JS_PAIR_LDS (sizeof(double) * (JS_W * JS_LD + 2 * JS_W * JS_LS + 3 * JS_B + 8))
#define JS_LEAD QRD_JSVD_LEAD               /* permutation entry: this column is the first of its cycle */

static_assert(JS_B == 32 && JS_CH % 16 == 0 && JS_LD % 32 == 2, "the LDS maps above assume blocks of 32 columns and a chunk leading dimension of 2 mod 32");
static_assert(JS_PAIR_LDS <= 160 * 1024, "a 128 x 64 chunk, S and J must fit one CU's LDS");

__device__ __forceinline__ v4d js_mfma(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// the maximum over the workgroup, the same value in every thread
__device__ __forceinline__ double js_block_max(double v, double* red, int t)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();                        // (red of an earlier call is read no more)
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// A pair of columns takes part in the measure and is rotated only if neither is negligible beside the other: |g_i| > eps |g_j| and
// the other way round.  A column below that changes its partner by less than an ulp; on an exactly rank-deficient matrix such a column
// is rounding noise that a sweep renews at 1e-15 of its own norm -- never orthogonal to tol, and without this test never converged.
__device__ __forceinline__ bool js_live(double a, double b)
{
    return a > 0.0 && b > 0.0 && a > (DBL_EPSILON * DBL_EPSILON) * b && b > (DBL_EPSILON * DBL_EPSILON) * a;
}

// max over the live pairs i < j of |s_ij| / sqrt(s_ii s_jj).  Ss[c * JS_LS + r] = S[r][c]
__device__ __forceinline__ double js_offdiag(const double* Ss, double* red, int t)
{
    double v = 0.0;
    for (int idx = t; idx < JS_W * JS_W; idx += 256) {
        const int i = idx & (JS_W - 1), j = idx >> 6;
        if (i < j) {
            const double a = Ss[i * JS_LS + i], b = Ss[j * JS_LS + j];
            if (js_live(a, b)) v = fmax(v, fabs(Ss[j * JS_LS + i]) / (sqrt(a) * sqrt(b)));
        }
    }
    return js_block_max(v, red, t);
}

// rows [row0, row0 + rows) of the pair's columns into the chunk image, zero for rows up to rows_pad and for columns that do not exist
__device__ __forceinline__ void js_load(double* Cs, const double* M, int ld, int row0, int rows, int rows_pad, int cp, int wp, int cq, int wq,
                                        int lane, int wv)
{
    for (int c = wv; c < JS_W; c += 4) {
        const int w = c & (JS_B - 1);
        const bool ok = c < JS_B ? w < wp : w < wq;
        const double* src = ok ? M + (size_t) ((c < JS_B ? cp : cq) + w) * ld + row0 : M;
        for (int i = lane; i < rows_pad; i += 64) Cs[c * JS_LD + i] = (ok && i < rows) ? src[i] : 0.0;
    }
}

__device__ __forceinline__ void js_store(const double* Cs, double* M, int ld, int row0, int rows, int cp, int wp, int cq, int wq, int lane, int wv)
{
    for (int c = wv; c < JS_W; c += 4) {
        const int w = c & (JS_B - 1);
        const bool ok = c < JS_B ? w < wp : w < wq;
        if (!ok) continue;
        double* dst = M + (size_t) ((c < JS_B ? cp : cq) + w) * ld + row0;
        for (int i = lane; i < rows; i += 64) dst[i] = Cs[c * JS_LD + i];
    }
}

// M(:, pair's columns) <- M(:, pair's columns) J over `total` rows in chunks; resident: the (single) chunk is in Cs already
__device__ __forceinline__ void js_apply(double* Cs, const double* Js, double* M, int ld, int total, bool resident, int cp, int wp, int cq, int wq,
                                         int lane, int wv)
{
    const int l15 = lane & 15, l4 = lane >> 4;
    for (int row0 = 0; row0 < total; row0 += JS_CH) {
        const int rows = min(JS_CH, total - row0), rp = (rows + 15) & ~15;
        if (!resident) {
            __syncthreads();                // (the stores of the previous chunk have read Cs)
            js_load(Cs, M, ld, row0, rows, rp, cp, wp, cq, wq, lane, wv);
        }
        __syncthreads();
        // wave wv: the 16-row tiles wv, wv + 4, ..: all four column tiles at once (they share the A operand); a tile's 16 x 64 result
        // depends on its own 16 rows only and goes back over them
        for (int rt = wv; rt < rp / 16; rt += 4) {
            v4d d0 = {0.0, 0.0, 0.0, 0.0}, d1 = d0, d2 = d0, d3 = d0;
#pragma unroll
            for (int ks = 0; ks < JS_W / 4; ++ks) {
                const int k = (ks & 7) + 8 * l4 + 32 * (ks >> 3);
                const double a = Cs[k * JS_LD + 16 * rt + l15];
                d0 = js_mfma(a, Js[l15 * JS_LS + k], d0);
                d1 = js_mfma(a, Js[(16 + l15) * JS_LS + k], d1);
                d2 = js_mfma(a, Js[(32 + l15) * JS_LS + k], d2);
                d3 = js_mfma(a, Js[(48 + l15) * JS_LS + k], d3);
            }
            double* o = Cs + l15 * JS_LD + 16 * rt + l4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[4 * r] = d0[r];
                o[16 * JS_LD + 4 * r] = d1[r];
                o[32 * JS_LD + 4 * r] = d2[r];
                o[48 * JS_LD + 4 * r] = d3[r];
            }
        }
        __syncthreads();
        js_store(Cs, M, ld, row0, rows, cp, wp, cq, wq, lane, wv);
    }
}

// the k-th of the 32 disjoint index pairs (i < j) of step st (0 .. 62) of a round-robin over 64 indices: 63 stays, the others turn
__device__ __forceinline__ void js_inner_pair(int st, int k, int& i, int& j)
{
    int a = k == 0 ? st : (st + k) % (JS_W - 1), b = k == 0 ? JS_W - 1 : (st - k + (JS_W - 1)) % (JS_W - 1);
    i = min(a, b);
    j = max(a, b);
}

__global__ void __launch_bounds__(256) jsvd_pair_kernel(double* __restrict__ G, int ldg, int r, int n, double* __restrict__ V, int ldv,
                                                        const int* __restrict__ pairs, double tol, double* __restrict__ slots)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* Cs = sm;                        // Cs[c * JS_LD + i] = chunk[i, c]
    double* Ss = Cs + JS_W * JS_LD;         // Ss[c * JS_LS + r] = S[r, c]
    double* Js = Ss + JS_W * JS_LS;         // Js[c * JS_LS + r] = J[r, c]
    double* cs = Js + JS_W * JS_LS;         // (cos, sin, 1 - cos) of the 32 rotations of a step
    double* red = cs + 3 * JS_B;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int bp = pairs[2 * blockIdx.x], bq = pairs[2 * blockIdx.x + 1];
    const int cp = bp * JS_B, wp = min(JS_B, n - cp);
    const int cq = bq * JS_B, wq = bq == bp ? 0 : min(JS_B, n - cq);
    const bool resident = r <= JS_CH;

    // 1. S = G_pq^T G_pq: wave wv owns the row of tiles wv, four MFMA chains (one per column tile) that run over all the rows in order
    {
        v4d a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0, a2 = a0, a3 = a0;
        for (int row0 = 0; row0 < r; row0 += JS_CH) {
            const int rows = min(JS_CH, r - row0), rp = (rows + 15) & ~15;
            if (row0) __syncthreads();      // (the previous chunk is read no more)
            js_load(Cs, G, ldg, row0, rows, rp, cp, wp, cq, wq, lane, wv);
            __syncthreads();
            const double* va = Cs + (16 * wv + l15) * JS_LD + l4;
            const double* vb = Cs + l15 * JS_LD + l4;
            for (int i = 0; i < rp; i += 4) {
                const double a = va[i];
                a0 = js_mfma(a, vb[i], a0);
                a1 = js_mfma(a, vb[16 * JS_LD + i], a1);
                a2 = js_mfma(a, vb[32 * JS_LD + i], a2);
                a3 = js_mfma(a, vb[48 * JS_LD + i], a3);
            }
        }
        double* o = Ss + l15 * JS_LS + 16 * wv + l4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o[4 * q] = a0[q];
            o[16 * JS_LS + 4 * q] = a1[q];
            o[32 * JS_LS + 4 * q] = a2[q];
            o[48 * JS_LS + 4 * q] = a3[q];
        }
    }
    __syncthreads();
    // S exactly symmetric: the upper triangle is the reference
    for (int idx = t; idx < JS_W * JS_W; idx += 256) {
        const int i = idx & (JS_W - 1), j = idx >> 6;
        if (i < j) Ss[i * JS_LS + j] = Ss[j * JS_LS + i];
    }
    __syncthreads();

    // 2. the pair's measure (the same value in every thread: the branch below is uniform)
    const double off = js_offdiag(Ss, red, t);
    if (t == 0) slots[blockIdx.x] = off;
    if (!(off > tol)) return;

    // 3. J = I, then cyclic sweeps of 63 steps x 32 disjoint rotations over S
    for (int idx = t; idx < JS_W * JS_W; idx += 256) Js[(idx >> 6) * JS_LS + (idx & (JS_W - 1))] = (idx >> 6) == (idx & (JS_W - 1)) ? 1.0 : 0.0;
    __syncthreads();
    for (int isw = 0; isw < JS_INNER_MAX; ++isw) {
        for (int st = 0; st < JS_W - 1; ++st) {
            if (t < JS_B) {
                int i, j;
                js_inner_pair(st, t, i, j);
                const double a = Ss[i * JS_LS + i], b = Ss[j * JS_LS + j], g = Ss[j * JS_LS + i];
                double c = 1.0, s = 0.0, h = 0.0;
                if (js_live(a, b) && fabs(g) > tol * (sqrt(a) * sqrt(b))) {
                    // columns i' = c i - s j, j' = s i + c j with tan^2 + 2 zeta tan - 1 = 0: the root of smaller modulus
                    const double zeta = (b - a) / (2.0 * g);
                    const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    c = 1.0 / sqrt(1.0 + tn * tn);
                    s = c * tn;
                    h = s * s / (1.0 + c);  // 1 - cos to full relative accuracy: see the J update below
                }
                cs[3 * t] = c;
                cs[3 * t + 1] = s;
                cs[3 * t + 2] = h;
            }
            __syncthreads();
            // S <- R^T S R on the 2 x 2 blocks (pa, pb), pa <= pb: a block is read and written by one thread, its mirror image written with it
            for (int idx = t; idx < JS_B * JS_B; idx += 256) {
                const int pa = idx >> 5, pb = idx & 31;
                if (pa > pb) continue;
                const double ca = cs[3 * pa], sa = cs[3 * pa + 1], cb = cs[3 * pb], sb = cs[3 * pb + 1];
                if (sa == 0.0 && sb == 0.0) continue;
                int ia, ja, ib, jb;
                js_inner_pair(st, pa, ia, ja);
                js_inner_pair(st, pb, ib, jb);
                const double m00 = Ss[ib * JS_LS + ia], m01 = Ss[jb * JS_LS + ia], m10 = Ss[ib * JS_LS + ja], m11 = Ss[jb * JS_LS + ja];
                const double t00 = cb * m00 - sb * m01, t01 = sb * m00 + cb * m01, t10 = cb * m10 - sb * m11, t11 = sb * m10 + cb * m11;
                const double n00 = ca * t00 - sa * t10, n01 = ca * t01 - sa * t11, n10 = sa * t00 + ca * t10, n11 = sa * t01 + ca * t11;
                if (pa == pb) {             // the rotated pair itself: its off-diagonal entry is zero by construction
                    Ss[ia * JS_LS + ia] = n00;
                    Ss[ja * JS_LS + ja] = n11;
                    Ss[ja * JS_LS + ia] = 0.0;
                    Ss[ia * JS_LS + ja] = 0.0;
                } else {
                    Ss[ib * JS_LS + ia] = n00; Ss[ia * JS_LS + ib] = n00;
                    Ss[jb * JS_LS + ia] = n01; Ss[ia * JS_LS + jb] = n01;
                    Ss[ib * JS_LS + ja] = n10; Ss[ja * JS_LS + ib] = n10;
                    Ss[jb * JS_LS + ja] = n11; Ss[ja * JS_LS + jb] = n11;
                }
            }
            // J <- J R with cos written as 1 - h: x' = x - (h x + s y), y' = y + (s x - h y).  A rounded cos is off by up to eps / 4, which
            // scales both columns by that much at every rotation; over the thousands of (mostly tiny) rotations a column of V passes
            // through, that walk -- not the angles -- was what cost V its unit column norms (36 n eps at n = 96 in the emulation, 1.7 so)
            for (int idx = t; idx < JS_B * JS_W; idx += 256) {
                const int pb = idx >> 6, x = idx & (JS_W - 1);
                const double sb = cs[3 * pb + 1], hb = cs[3 * pb + 2];
                if (sb == 0.0) continue;
                int ib, jb;
                js_inner_pair(st, pb, ib, jb);
                const double ji = Js[ib * JS_LS + x], jj = Js[jb * JS_LS + x];
                Js[ib * JS_LS + x] = ji - (hb * ji + sb * jj);
                Js[jb * JS_LS + x] = jj + (sb * ji - hb * jj);
            }
            __syncthreads();
        }
        if (!(js_offdiag(Ss, red, t) > tol)) break;
    }

    // 4. G_pq <- G_pq J, V_pq <- V_pq J
    js_apply(Cs, Js, G, ldg, r, resident, cp, wp, cq, wq, lane, wv);
    if (V) js_apply(Cs, Js, V, ldv, n, false, cp, wp, cq, wq, lane, wv);
}

__global__ void __launch_bounds__(256) jsvd_fold_kernel(const double* __restrict__ slots, int count, double* __restrict__ word)
{
    __shared__ double red[4];
    const int t = threadIdx.x;
    double v = 0.0;
    for (int i = t; i < count; i += 256) v = fmax(v, slots[i]);
    v = js_block_max(v, red, t);
    if (t == 0) word[0] = v;
}

// out[c] = |X(0:rows, c)|, c = blockIdx.x: thread-strided partial sums, a wave butterfly, the four waves in wave order
__global__ void __launch_bounds__(256) jsvd_colnorm_kernel(const double* __restrict__ X, int ldx, int rows, double* __restrict__ out)
{
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double* x = X + (size_t) blockIdx.x * ldx;
    double s = 0.0;
    for (int i = t; i < rows; i += 256) s = fma(x[i], x[i], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) out[blockIdx.x] = sqrt(((red[0] + red[1]) + red[2]) + red[3]);
}

__global__ void jsvd_gather_kernel(const double* __restrict__ sig, const int* __restrict__ perm, double* __restrict__ out, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = sig[perm[j] & (JS_LEAD - 1)];
}

// column j <- column perm[j] of M (rows x n), in place: one thread per row walks every cycle of the permutation from its first column
// (flagged JS_LEAD by the host), one element in a register; each element is read once and written once
__global__ void __launch_bounds__(256) jsvd_permute_kernel(double* __restrict__ M, int ld, int rows, int n, const int* __restrict__ perm)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    double* row = M + i;
    for (int j = 0; j < n; ++j) {
        const int pj = perm[j];
        int src = pj & (JS_LEAD - 1);
        if (!(pj & JS_LEAD) || src == j) continue;
        const double first = row[(size_t) j * ld];
        int k = j;
        for (int guard = 0; guard < n && src != j; ++guard) {      // (a cycle has at most n columns)
            row[(size_t) k * ld] = row[(size_t) src * ld];
            k = src;
            src = perm[k] & (JS_LEAD - 1);
        }
        row[(size_t) k * ld] = first;
    }
}

__global__ void jsvd_normalise_kernel(double* __restrict__ X, int ldx, int rows, const double* __restrict__ sig)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double s = sig[blockIdx.y];
    if (i < rows && s > 0.0) X[(size_t) blockIdx.y * ldx + i] /= s;
}

// T2[i, j] = T1[i, j] / sig[i] where sig[i] > rc sig[0], else 0 (both n x nrhs, ld n)
__global__ void jsvd_pinv_kernel(const double* __restrict__ T1, double* __restrict__ T2, int n, const double* __restrict__ sig, double rc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s = sig[i];
    const size_t at = (size_t) blockIdx.y * n + i;
    T2[at] = s > rc * sig[0] ? T1[at] / s : 0.0;
}

// W (n x n, ldw) = R^T: W[i, j] = A[j, i] for i >= j, zero above the diagonal
__global__ void jsvd_rt_kernel(const double* __restrict__ A, int lda, int n, double* __restrict__ W, int ldw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i < n) W[(size_t) j * ldw + i] = i >= j ? A[(size_t) i * lda + j] : 0.0;
}

// the kernel that asks for more than 64 KiB of LDS (qr_allow_lds)
static int js_allow_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(jsvd_pair_kernel)};
    return qr_allow_lds(fns, (int) JS_PAIR_LDS, done);
}

extern "C" {

int qrd_jsvd_round(void* stream, double* G, int ldg, int r, int n, double* V, int ldv, const int* pairs, int npairs, double tol, double* slots)
{
    if (npairs <= 0) return 0;
    if (r < 1 || n < 1 || ldg < r || (V && ldv < n) || !pairs || !slots) return -7;
    const int rc = js_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(jsvd_pair_kernel, dim3((unsigned) npairs), dim3(256), JS_PAIR_LDS, (hipStream_t) stream, G, ldg, r, n, V, ldv, pairs, tol,
                       slots);
    return (int) hipGetLastError();
}

int qrd_jsvd_fold(void* stream, const double* slots, int count, double* word)
{
    hipLaunchKernelGGL(jsvd_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t) stream, slots, count, word);
    return (int) hipGetLastError();
}

int qrd_jsvd_colnorms(void* stream, const double* G, int ldg, int r, int n, double* out)
{
    if (r <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(jsvd_colnorm_kernel, dim3((unsigned) n), dim3(256), 0, (hipStream_t) stream, G, ldg, r, out);
    return (int) hipGetLastError();
}

int qrd_jsvd_gather(void* stream, const double* sig, const int* perm, double* out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(jsvd_gather_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, sig, perm, out, n);
    return (int) hipGetLastError();
}

int qrd_jsvd_permute(void* stream, double* M, int ld, int rows, int n, const int* perm)
{
    if (rows <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(jsvd_permute_kernel, dim3((unsigned) ((rows + 255) / 256)), dim3(256), 0, (hipStream_t) stream, M, ld, rows, n, perm);
    return (int) hipGetLastError();
}

int qrd_jsvd_normalise(void* stream, double* G, int ldg, int r, int n, const double* sig)
{
    if (r <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(jsvd_normalise_kernel, dim3((unsigned) ((r + 255) / 256), (unsigned) n), dim3(256), 0, (hipStream_t) stream, G, ldg, r, sig);
    return (int) hipGetLastError();
}

int qrd_jsvd_pinv_scale(void* stream, const double* T1, double* T2, int n, int nrhs, const double* sig, double rc)
{
    if (n <= 0 || nrhs <= 0) return 0;
    hipLaunchKernelGGL(jsvd_pinv_kernel, dim3((unsigned) ((n + 255) / 256), (unsigned) nrhs), dim3(256), 0, (hipStream_t) stream, T1, T2, n, sig, rc);
    return (int) hipGetLastError();
}

int qrd_jsvd_rt(void* stream, const double* A, int lda, int n, double* W, int ldw)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(jsvd_rt_kernel, dim3((unsigned) ((n + 255) / 256), (unsigned) n), dim3(256), 0, (hipStream_t) stream, A, lda, n, W, ldw);
    return (int) hipGetLastError();
}

}   // extern "C"
