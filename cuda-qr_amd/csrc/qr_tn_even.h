/* qr_tn_even.h -- the even, static K split of the wide TN product Wt = A2^T (V T), as plain integer arithmetic shared by the
 * launch code, the kernels (qr_kernels.hip) and a host-side checker (tests/c/tn_even_check.c).  No HIP types.
 *
 * The work is the list of (tile, k-tile) units, tile-major: unit u = tile * nkt + kt, U = tiles * nkt of them.  G workgroups are
 * launched; workgroup g owns the units [floor(g U / G), floor((g + 1) U / G)), so no two workgroups differ by more than one unit.
 * A workgroup's range is cut at tile boundaries into segments (tile, first k-tile, k-tile count, slot); a segment's 128 x 128
 * partial sum goes to partial-tile slot `slot` of the slab buffer.
 *
 *   slot = tile + rank(g),   rank(g) = number of non-empty workgroups before g = min(g, floor(g U / G))
 *
 * (U >= G: every workgroup owns a unit, rank = g.  U < G: a workgroup owns one unit or none, so the non-empty ones before g are as
 * many as the units before g.)  Walking the segments in (workgroup, tile) order, each next segment raises the tile, the rank or
 * both, so slots are unique, below G + tiles, and those of one tile are consecutive and ascending in k: the reduce sums slots
 * [first, first + count) of a tile in that order.  Nothing here depends on what another workgroup does. */
#ifndef QR_TN_EVEN_H
#define QR_TN_EVEN_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QR_TN_EVEN_FN __host__ __device__ static inline
#else
#define QR_TN_EVEN_FN static inline
#endif

typedef struct { int tile, kt0, nkt, slot; } tn_even_seg;

/* first unit of workgroup g (g = G gives U); U = tiles * nkt must be below 2^31 */
QR_TN_EVEN_FN int tn_even_unit0(int g, int G, int U) { return (int) ((long long) g * U / G); }

/* non-empty workgroups before g */
QR_TN_EVEN_FN int tn_even_rank(int g, int G, int U)
{
    const int u0 = tn_even_unit0(g, G, U);
    return g < u0 ? g : u0;
}

/* the segment of workgroup g (rank = tn_even_rank(g)) that starts at unit u of its range [.., u1): up to the end of u's tile or of the range */
QR_TN_EVEN_FN tn_even_seg tn_even_seg_at(int u, int u1, int nkt, int rank)
{
    tn_even_seg s;
    s.tile = u / nkt;
    s.kt0 = u - s.tile * nkt;
    s.nkt = nkt - s.kt0 < u1 - u ? nkt - s.kt0 : u1 - u;
    s.slot = s.tile + rank;
    return s;
}

/* the workgroup that owns unit u: the smallest g with floor((g + 1) U / G) > u */
QR_TN_EVEN_FN int tn_even_owner(int u, int G, int U) { return (int) ((((long long) u + 1) * G + U - 1) / U) - 1; }

/* the reduce's view: the partial tiles of `tile` are slots [*first, *first + *count), ascending in k */
QR_TN_EVEN_FN void tn_even_tile_slots(int tile, int G, int tiles, int nkt, int* first, int* count)
{
    const int U = tiles * nkt;
    const int ra = tn_even_rank(tn_even_owner(tile * nkt, G, U), G, U);
    const int rb = tn_even_rank(tn_even_owner(tile * nkt + nkt - 1, G, U), G, U);
    *first = tile + ra;
    *count = rb - ra + 1;
}

#endif
