// qr_update.hip -- kernels of the row-append update (qr_update.c, mi355x_qr.h section 6) and of the signed-row update (qr_downdate.c,
// section 6b): QR of a triangle R stacked on a block B of rows.  One family, two instances of each body, selected at compile time:
// the unsigned one (tp_*) adds every row; the signed one (th_*, Signed below) adds the block's first p_add rows and removes its last
// p - p_add, R'^T R' = R^T R + B^T S B, S = diag(+1 .. +1, -1 .. -1).
//
//   tp_panel_kernel    one workgroup factors [R_kk (w x w triangle) ; B(:, k:k+w)] column by column with the B panel resident in LDS
//   tp_apply_kernel    one workgroup per slab of 32 columns: W = op(T_k) (C1 + V_k^T C2), C1 -= W, C2 -= V_k W on v_mfma_f64_16x16x4_f64
//   tp_colssq_kernel   per-column sum of squares of a block, added into device accumulators (one workgroup per column, fixed order)
//   tp_sqrt_kernel     out[i] = sqrt(in[i])
//   th_panel_kernel    the panel with every inner product over the block's rows weighted by S, and the test of d = R(j,j)^2 + b^T S b
//                      that ends the call when no positive-definite triangle is left
//   th_apply_kernel    W = T_k^T (C1 + V_k^T S C2), C1 -= W, C2 -= V_k W
//   th_colssq_kernel   acc[c] = max(0, acc[c] + |X(0:p_add, c)|^2 - |X(p_add:p, c)|^2)
//
// Reflector j of a panel is [e_j ; V(:, j)]: the identity on top is never stored or multiplied.  With it V_full^T C = C1 + V^T C2 and
// V_full W = [W ; V W], which is all the apply kernel computes.  Signed, reflector j is Theta_j = I - tau_j u_j u_j^T Phi,
// u_j = [e_j ; V(:, j)], Phi = diag(I, S): only the products that contract over the block's rows see S (V^T S C2, V^T S V); the rank-one
// and rank-w corrections V w, V W do not.
//
// LDS images (both kernels): a p x 32 block is kept column-major with a leading dimension of TP_LD = 258 doubles.  8-byte accesses are
// served per 32-lane half, bank = (byte address / 4) mod 64, two banks per double, so a half is conflict-free when its 32 double
// indices are distinct mod 32.  The MFMA operand reads are of two kinds:
//   (lane & 15) along the block's columns, (lane >> 4) along its rows (V^T C2: both operands; the C2 accumulator tiles):
//       index = (lane & 15) * 258 + (lane >> 4) + const = 2 (lane & 15) + {0, 1} (mod 32) -- 32 distinct values;
//   (lane & 15) along the rows, (lane >> 4) along the columns (V as the A operand of V W): the four k of a step are taken 8 columns
//       apart (k-step s = columns s, s + 8, s + 16, s + 24; the B operand W uses the same map), so a half reads rows r .. r + 15 of
//       columns c and c + 8: index = (lane & 15) + {0, 8 * 258 = 16 (mod 32)} -- 32 distinct values.
// The 32 x 32 matrices (R_kk, T_k, W) have a leading dimension of 33.  S costs no access: it is applied to the V operand of V^T S C2
// (and to v_j in the panel's dot products) in the register it was read into, by the row index the lane already holds (row >= p_add:
// negate).  It is one product, not two, and the same addresses in the same order.
//
// Fragment maps of v_mfma_f64_16x16x4_f64: A operand lane l = A[row l & 15][k l >> 4], B operand lane l = B[k l >> 4][col l & 15],
// C / D register r of lane l = D[row (l >> 4) + 4 r][col l & 15].
//
// The status word of the signed instances: one device int, 0 while all is well.  Each of them reads it before anything else and returns
// when it is set (the same value in every thread, so whole workgroups leave together, before any barrier).  Only th_panel_kernel writes
// it -- one workgroup, one thread, a plain vector store of the failing global column + 1 -- and launches of one call are ordered on one
// stream, so the first failure is the only one recorded.
//
// Every sum runs in a fixed order (wave butterflies, waves added in wave order, MFMA chains in k order): repeated launches give
// bitwise-equal results.  No atomics.
#include "qr_common.h"
#include "qr_device.h"

#define TP_W QRD_TP_W
#define TP_P QRD_TP_MAXROWS
#define TP_LD (TP_P + 2)
#define TP_LT (TP_W + 1)
#define TP_PANEL_LDS (sizeof(double) * (TP_W * TP_LD + 2 * TP_W * TP_LT + TP_W + 8))
#define TP_APPLY_LDS (sizeof(double) * (2 * TP_W * TP_LD + 3 * TP_W * TP_LT))

static_assert(TP_W == 32 && TP_P % 16 == 0 && TP_LD % 32 == 2, "the LDS maps above assume 32 columns and a leading dimension of 2 mod 32");
static_assert(TP_P <= 256, "the signed instances give one block row to each thread");
static_assert(TP_APPLY_LDS <= 160 * 1024, "the apply kernel's V panel, C2 slab, T and two W tiles must fit one CU's LDS");

// the same sum in every lane; the order of the additions does not depend on the data
__device__ __forceinline__ double tp_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the four waves' sums, in wave order
__device__ __forceinline__ double tp_sum4(const double* red) { return ((red[0] + red[1]) + red[2]) + red[3]; }

// [R (w x w upper triangle, ldr) ; B (p x w, ldb)] = Q [R' ; 0]: R' over R's triangle (the strict lower triangle is neither read nor
// written), V over B, the w x w upper-triangular T (zeros below its diagonal) to T (ldt).  LAPACK dlarfg per column: beta =
// -sign(alpha) hypot(alpha, |x|), tau = (beta - alpha) / beta, v = x / (alpha - beta); x == 0 exactly: tau = 0, nothing changes.
// An exact zero of B stays an exact zero (v = 0 there, and the update adds -tau w * 0).
// Signed: -> [R' ; 0] under the signs S.  Thread t owns row t of the block.  Per column, with sa / sd the sums of squares of the added /
// removed rows: h = hypot(alpha, sqrt(sa)), d = (h - sqrt(sd)) (h + sqrt(sd)) -- the difference of squares is never formed --,
// beta = -sign(alpha) sqrt(d); d <= 0 or not finite: *status = col0 + j + 1, and the launch ends without writing anything back.
// (p_add, col0 and status are the signed instance's.)
template <bool Signed>
__device__ __forceinline__ void tp_panel_body(double* __restrict__ R, int ldr, double* __restrict__ B, int ldb, int p, int p_add, int w,
                                              double* __restrict__ T, int ldt, int col0, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if constexpr (Signed)
        if (*status != 0) return;
    double* Bs = sm;                        // Bs[c * TP_LD + i] = B[i, c]
    double* Rs = Bs + TP_W * TP_LD;         // Rs[c * TP_LT + r] = R[r, c], r <= c
    double* Ts = Rs + TP_W * TP_LT;         // Ts[c * TP_LT + r] = T[r, c]
    double* dots = Ts + TP_W * TP_LT;       // V[:, c]^T (S) v_j, c < j
    double* red = dots + TP_W;              // 4 partial sums (Signed: of the added rows, and 4 of the removed ones)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int c = wv; c < w; c += 4)
        for (int i = lane; i < p; i += 64) Bs[c * TP_LD + i] = B[(size_t) c * ldb + i];
    for (int idx = t; idx < TP_W * TP_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        Rs[c * TP_LT + r] = (r <= c && c < w) ? R[(size_t) c * ldr + r] : 0.0;
        Ts[c * TP_LT + r] = 0.0;
    }
    __syncthreads();
    for (int j = 0; j < w; ++j) {
        double* vj = Bs + j * TP_LD;
        double x = 0.0, sa, sd = 0.0;       // (x: this thread's row of column j, sd: Signed only)
        if constexpr (Signed) {             // its square goes to the sum of its sign
            x = t < p ? vj[t] : 0.0;
            const double x2 = x * x;
            const double sa_w = tp_wave_sum(t < p_add ? x2 : 0.0), sd_w = tp_wave_sum(t < p_add ? 0.0 : x2);
            if (lane == 0) { red[wv] = sa_w; red[4 + wv] = sd_w; }
            __syncthreads();
            sa = tp_sum4(red);
            sd = tp_sum4(red + 4);
        } else {
            double s = 0.0;
            for (int i = t; i < p; i += 256) s = fma(vj[i], vj[i], s);
            s = tp_wave_sum(s);
            if (lane == 0) red[wv] = s;
            __syncthreads();
            sa = tp_sum4(red);
        }
        if (sa != 0.0 || sd != 0.0) {       // (the same values in every thread)
            const double alpha = Rs[j * TP_LT + j];
            // (nd and d are the signed instance's and dead in the other.  Declared flat on purpose: with beta assigned inside the branch
            // below hipcc gave th_panel_kernel 48 VGPRs for the 46 it has this way.)
            const double h = hypot(alpha, sqrt(sa)), nd = sqrt(sd), d = (h - nd) * (h + nd);
            if constexpr (Signed)
                if (!(d > 0.0) || !isfinite(d)) {
                    if (t == 0) *status = col0 + j + 1;
                    return;
                }
            const double beta = -copysign(Signed ? sqrt(d) : h, alpha);
            const double tau = (beta - alpha) / beta, scal = 1.0 / (alpha - beta);
            if constexpr (Signed) {
                if (t < p) vj[t] = x * scal;
            } else
                for (int i = t; i < p; i += 256) vj[i] *= scal;
            __syncthreads();
            if (t == 0) Rs[j * TP_LT + j] = beta;
            // wave wv: columns wv, wv + 4, ..: the (signed) dot product with v_j, then (to the right of j) that column's update
            for (int c = wv; c < w; c += 4) {
                if (c == j) continue;
                double* bc = Bs + c * TP_LD;
                double dt = 0.0;
                for (int i = lane; i < p; i += 64) {
                    if constexpr (Signed) dt = fma(i < p_add ? vj[i] : -vj[i], bc[i], dt);
                    else dt = fma(vj[i], bc[i], dt);
                }
                dt = tp_wave_sum(dt);
                if (c < j) {
                    if (lane == 0) dots[c] = dt;
                } else {
                    const double tw = tau * (Rs[c * TP_LT + j] + dt);
                    if (lane == 0) Rs[c * TP_LT + j] -= tw;
                    for (int i = lane; i < p; i += 64) bc[i] = fma(-tw, vj[i], bc[i]);
                }
            }
            __syncthreads();
            // T[0:j, j] = -tau T[0:j, 0:j] (V[:, 0:j]^T (S) v_j), T[j, j] = tau (dlarft, forward columnwise; the unit tops are orthogonal)
            if (t < j) {
                double a = 0.0;
                for (int l = t; l < j; ++l) a = fma(Ts[l * TP_LT + t], dots[l], a);
                Ts[j * TP_LT + t] = -tau * a;
            } else if (t == j) Ts[j * TP_LT + j] = tau;
        }
        __syncthreads();                    // (red, dots and column j are read no more)
    }
    for (int c = wv; c < w; c += 4)
        for (int i = lane; i < p; i += 64) B[(size_t) c * ldb + i] = Bs[c * TP_LD + i];
    for (int idx = t; idx < TP_W * TP_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        if (c < w && r < w) {
            if (r <= c) R[(size_t) c * ldr + r] = Rs[c * TP_LT + r];
            T[(size_t) c * ldt + r] = Ts[c * TP_LT + r];
        }
    }
}

__global__ void __launch_bounds__(256) tp_panel_kernel(double* __restrict__ R, int ldr, double* __restrict__ B, int ldb, int p, int w,
                                                       double* __restrict__ T, int ldt)
{
    tp_panel_body<false>(R, ldr, B, ldb, p, p, w, T, ldt, 0, nullptr);
}

__global__ void __launch_bounds__(256) th_panel_kernel(double* __restrict__ R, int ldr, double* __restrict__ B, int ldb, int p, int p_add, int w,
                                                       double* __restrict__ T, int ldt, int col0, int* __restrict__ status)
{
    tp_panel_body<true>(R, ldr, B, ldb, p, p_add, w, T, ldt, col0, status);
}

__device__ __forceinline__ v4d tp_mfma(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// Columns [32 b, 32 b + 32) of C (b = blockIdx.x; ncols in all):  W = op(T) (C1 + V^T C2), C1 -= W, C2 -= V W  with V p x w (ldv),
// T w x w upper triangular (ldt; what lies below its diagonal is not read), C1 w x ncols (ldc1), C2 p x ncols (ldc2);
// tr != 0: op(T) = T^T (Q'^T C), else T (Q' C).  V and the C2 slab are staged in LDS with the lanes along a column (contiguous global
// accesses, any leading dimension or base); the slab goes back the same way: C2 is read once and written once.
// Signed: W = T^T (C1 + V^T S C2), whatever tr is (p_add and status are the signed instance's).
template <bool Signed>
__device__ __forceinline__ void tp_apply_body(int tr, const double* __restrict__ V, int ldv, int p, int p_add, int w, const double* __restrict__ T,
                                              int ldt, double* __restrict__ C1, int ldc1, double* __restrict__ C2, int ldc2, int ncols,
                                              const int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if constexpr (Signed)
        if (*status != 0) return;
    double* Vs = sm;                        // Vs[c * TP_LD + i] = V[i, c], zero for i >= p or c >= w
    double* Cs = Vs + TP_W * TP_LD;         // Cs[c * TP_LD + i] = C2[i, c0 + c], zero outside
    double* Ts = Cs + TP_W * TP_LD;         // Ts[c * TP_LT + r] = T[r, c]
    double* W0 = Ts + TP_W * TP_LT;         // W0[c * TP_LT + r] = (C1 + V^T (S) C2)[r, c]
    double* W1 = W0 + TP_W * TP_LT;         // W
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int c0 = (int) blockIdx.x * TP_W, nc = min(TP_W, ncols - c0), p16 = (p + 15) & ~15;
    C1 += (size_t) c0 * ldc1;
    C2 += (size_t) c0 * ldc2;
    for (int c = wv; c < TP_W; c += 4)
        for (int i = lane; i < p16; i += 64) {
            Vs[c * TP_LD + i] = (c < w && i < p) ? V[(size_t) c * ldv + i] : 0.0;
            Cs[c * TP_LD + i] = (c < nc && i < p) ? C2[(size_t) c * ldc2 + i] : 0.0;
        }
    for (int idx = t; idx < TP_W * TP_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        Ts[c * TP_LT + r] = (r <= c && c < w) ? T[(size_t) c * ldt + r] : 0.0;
    }
    __syncthreads();
    // 1. wave wv: the 16 x 16 tile (ti, tj) of V^T (S) C2, K = p16 in four interleaved chains added in a fixed order.  Signed: this
    // lane's V operand of chain q at step i is row i + 4 q + l4 of the block: negated from row p_add on.
    const int ti = wv & 1, tj = wv >> 1;
    const int row0 = 16 * ti + l4, col = 16 * tj + l15;        // this lane's D entries: rows row0 + 4 r, column col
    v4d c1v, w0v;
    {
        const double* va = Vs + (16 * ti + l15) * TP_LD + l4;
        const double* cb = Cs + col * TP_LD + l4;
        const int pa = p_add - l4;                             // row i + 4 q + l4 < p_add  <=>  i + 4 q < pa
        v4d a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0, a2 = a0, a3 = a0;
        for (int i = 0; i < p16; i += 16) {
            if constexpr (Signed) {
                a0 = tp_mfma(i < pa ? va[i] : -va[i], cb[i], a0);
                a1 = tp_mfma(i + 4 < pa ? va[i + 4] : -va[i + 4], cb[i + 4], a1);
                a2 = tp_mfma(i + 8 < pa ? va[i + 8] : -va[i + 8], cb[i + 8], a2);
                a3 = tp_mfma(i + 12 < pa ? va[i + 12] : -va[i + 12], cb[i + 12], a3);
            } else {
                a0 = tp_mfma(va[i], cb[i], a0);
                a1 = tp_mfma(va[i + 4], cb[i + 4], a1);
                a2 = tp_mfma(va[i + 8], cb[i + 8], a2);
                a3 = tp_mfma(va[i + 12], cb[i + 12], a3);
            }
        }
        const v4d acc = (a0 + a1) + (a2 + a3);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r;
            c1v[r] = (row < w && col < nc) ? C1[(size_t) col * ldc1 + row] : 0.0;
            w0v[r] = acc[r] + c1v[r];
            W0[col * TP_LT + row] = w0v[r];
        }
    }
    __syncthreads();
    // 2. W = op(T) W0, the same tile; C1 -= W
    {
        v4d wacc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < TP_W / 4; ++ks) {
            const int k = 4 * ks + l4, ar = 16 * ti + l15;
            const double a = (Signed || tr) ? Ts[ar * TP_LT + k] : Ts[k * TP_LT + ar];
            wacc = tp_mfma(a, W0[col * TP_LT + k], wacc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r;
            W1[col * TP_LT + row] = wacc[r];
            if (row < w && col < nc) C1[(size_t) col * ldc1 + row] = c1v[r] - wacc[r];
        }
    }
    __syncthreads();
    // 3. C2 -= V W (no signs: the correction is along u_j, not Phi u_j): wave wv takes the 16-row tiles wv, wv + 4, .. of the slab, both
    // column tiles at once (they share the A operand); k-step ks = columns ks, ks + 8, ks + 16, ks + 24 of V (see the bank note above)
    for (int rt = wv; rt < p16 / 16; rt += 4) {
        double* d0p = Cs + l15 * TP_LD + 16 * rt + l4;
        double* d1p = d0p + 16 * TP_LD;
        v4d d0, d1;
#pragma unroll
        for (int r = 0; r < 4; ++r) { d0[r] = d0p[4 * r]; d1[r] = d1p[4 * r]; }
#pragma unroll
        for (int ks = 0; ks < TP_W / 4; ++ks) {
            const int c = ks + 8 * l4;
            const double a = -Vs[c * TP_LD + 16 * rt + l15];
            d0 = tp_mfma(a, W1[l15 * TP_LT + c], d0);
            d1 = tp_mfma(a, W1[(16 + l15) * TP_LT + c], d1);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) { d0p[4 * r] = d0[r]; d1p[4 * r] = d1[r]; }
    }
    __syncthreads();
    for (int c = wv; c < nc; c += 4)
        for (int i = lane; i < p; i += 64) C2[(size_t) c * ldc2 + i] = Cs[c * TP_LD + i];
}

__global__ void __launch_bounds__(256) tp_apply_kernel(int tr, const double* __restrict__ V, int ldv, int p, int w, const double* __restrict__ T,
                                                       int ldt, double* __restrict__ C1, int ldc1, double* __restrict__ C2, int ldc2, int ncols)
{
    tp_apply_body<false>(tr, V, ldv, p, p, w, T, ldt, C1, ldc1, C2, ldc2, ncols, nullptr);
}

__global__ void __launch_bounds__(256) th_apply_kernel(const double* __restrict__ V, int ldv, int p, int p_add, int w, const double* __restrict__ T,
                                                       int ldt, double* __restrict__ C1, int ldc1, double* __restrict__ C2, int ldc2, int ncols,
                                                       const int* __restrict__ status)
{
    tp_apply_body<true>(1, V, ldv, p, p_add, w, T, ldt, C1, ldc1, C2, ldc2, ncols, status);
}

// acc[c] += sum over i < rows of X[i, c]^2, c = blockIdx.x: thread-strided partial sums, a wave butterfly, the four waves in wave order
__global__ void __launch_bounds__(256) tp_colssq_kernel(const double* __restrict__ X, int ldx, int rows, double* __restrict__ acc)
{
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double* x = X + (size_t) blockIdx.x * ldx;
    double s = 0.0;
    for (int i = t; i < rows; i += 256) s = fma(x[i], x[i], s);
    s = tp_wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) acc[blockIdx.x] += tp_sum4(red);
}

// acc[c] = max(0, acc[c] + sum over i < p_add of X[i, c]^2 - sum over p_add <= i < p of X[i, c]^2), c = blockIdx.x, p <= 256: one row per
// thread, two wave butterflies, the four waves in wave order
__global__ void __launch_bounds__(256) th_colssq_kernel(const double* __restrict__ X, int ldx, int p, int p_add, double* __restrict__ acc,
                                                        const int* __restrict__ status)
{
    __shared__ double red[8];
    if (*status != 0) return;
    const int t = threadIdx.x;
    const double x = t < p ? X[(size_t) blockIdx.x * ldx + t] : 0.0, x2 = x * x;
    const double sa = tp_wave_sum(t < p_add ? x2 : 0.0), sd = tp_wave_sum(t < p_add ? 0.0 : x2);
    if ((t & 63) == 0) { red[t >> 6] = sa; red[4 + (t >> 6)] = sd; }
    __syncthreads();
    if (t == 0) {
        const double a = tp_sum4(red), d = tp_sum4(red + 4);
        acc[blockIdx.x] = fmax(0.0, (acc[blockIdx.x] + a) - d);
    }
}

__global__ void tp_sqrt_kernel(const double* __restrict__ in, double* __restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sqrt(in[i]);
}

// the kernels that ask for more than 64 KiB of LDS (qr_allow_lds): the two panels, the two applies
static int tp_allow_panel_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(tp_panel_kernel), reinterpret_cast<const void*>(th_panel_kernel)};
    return qr_allow_lds(fns, (int) TP_PANEL_LDS, done);
}

static int tp_allow_apply_lds(void)
{
    static std::atomic<int> done[64];
    const void* const fns[] = {reinterpret_cast<const void*>(tp_apply_kernel), reinterpret_cast<const void*>(th_apply_kernel)};
    return qr_allow_lds(fns, (int) TP_APPLY_LDS, done);
}

extern "C" {

int qrd_tp_panel(void* stream, double* Rkk, int ldr, double* Bk, int ldb, int p, int w, double* Tk, int ldt)
{
    if (p < 1 || p > TP_P || w < 1 || w > TP_W || ldr < w || ldb < p || ldt < w) return -7;
    const int rc = tp_allow_panel_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(tp_panel_kernel, dim3(1), dim3(256), TP_PANEL_LDS, (hipStream_t) stream, Rkk, ldr, Bk, ldb, p, w, Tk, ldt);
    return (int) hipGetLastError();
}

int qrd_tp_apply(void* stream, int trans_t, const double* Vk, int ldv, int p, int w, const double* Tk, int ldt, double* C1k, int ldc1,
                 double* C2, int ldc2, int ncols)
{
    if (ncols <= 0) return 0;
    if (p < 1 || p > TP_P || w < 1 || w > TP_W || ldv < p || ldt < w || ldc1 < w || ldc2 < p) return -7;
    const int rc = tp_allow_apply_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(tp_apply_kernel, dim3((unsigned) ((ncols + TP_W - 1) / TP_W)), dim3(256), TP_APPLY_LDS, (hipStream_t) stream,
                       trans_t, Vk, ldv, p, w, Tk, ldt, C1k, ldc1, C2, ldc2, ncols);
    return (int) hipGetLastError();
}

int qrd_tp_colssq_add(void* stream, const double* X, int ldx, int rows, int cols, double* acc)
{
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(tp_colssq_kernel, dim3((unsigned) cols), dim3(256), 0, (hipStream_t) stream, X, ldx, rows, acc);
    return (int) hipGetLastError();
}

int qrd_tp_sqrt(void* stream, const double* in, double* out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(tp_sqrt_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, in, out, n);
    return (int) hipGetLastError();
}

int qrd_th_panel(void* stream, double* Rkk, int ldr, double* Bk, int ldb, int p, int p_add, int w, double* Tk, int ldt, int col0, int* status)
{
    if (p < 1 || p > TP_P || p_add < 0 || p_add > p || w < 1 || w > TP_W || ldr < w || ldb < p || ldt < w || col0 < 0 || !status) return -7;
    const int rc = tp_allow_panel_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(th_panel_kernel, dim3(1), dim3(256), TP_PANEL_LDS, (hipStream_t) stream, Rkk, ldr, Bk, ldb, p, p_add, w, Tk, ldt, col0,
                       status);
    return (int) hipGetLastError();
}

int qrd_th_apply(void* stream, const double* Vk, int ldv, int p, int p_add, int w, const double* Tk, int ldt, double* C1k, int ldc1,
                 double* C2, int ldc2, int ncols, const int* status)
{
    if (ncols <= 0) return 0;
    if (p < 1 || p > TP_P || p_add < 0 || p_add > p || w < 1 || w > TP_W || ldv < p || ldt < w || ldc1 < w || ldc2 < p || !status) return -7;
    const int rc = tp_allow_apply_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(th_apply_kernel, dim3((unsigned) ((ncols + TP_W - 1) / TP_W)), dim3(256), TP_APPLY_LDS, (hipStream_t) stream,
                       Vk, ldv, p, p_add, w, Tk, ldt, C1k, ldc1, C2, ldc2, ncols, status);
    return (int) hipGetLastError();
}

int qrd_th_colssq(void* stream, const double* X, int ldx, int p, int p_add, int cols, double* acc, const int* status)
{
    if (cols <= 0) return 0;
    if (p < 1 || p > TP_P || p_add < 0 || p_add > p || ldx < p || !status) return -7;
    hipLaunchKernelGGL(th_colssq_kernel, dim3((unsigned) cols), dim3(256), 0, (hipStream_t) stream, X, ldx, p, p_add, acc, status);
    return (int) hipGetLastError();
}

}   // extern "C"
