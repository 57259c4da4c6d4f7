/* tn_even_check.c -- TEST-ONLY stand-alone checker of the even K split's index arithmetic (cuda-qr_amd/csrc/qr_tn_even.h), built with
 * the host compiler by tests/test_tn_even_split.py (optionally with -fsanitize=address,undefined).  For every (tiles, k-tiles, G):
 *   - the segments cover every (tile, k-tile) unit exactly once and no segment crosses a tile;
 *   - the segments of a tile are consecutive in slot order and ascending in k;
 *   - slots are unique and below G + tiles;
 *   - tn_even_tile_slots() (what the reduce uses) names exactly the slots the product wrote for that tile;
 *   - workgroups with an empty range own no slot.
 * Prints "tn_even_check ok <triples>" and exits 0, or the first failing triple and exits 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../cuda-qr_amd/csrc/qr_tn_even.h"

#define MAX_TILES 256
#define MAX_G 512
#define MAX_UNITS 1600
#define FAIL(msg) do { fprintf(stderr, "tn_even_check: %s (tiles %d, nkt %d, G %d, g %d)\n", msg, tiles, nkt, G, g); return 1; } while (0)

/* per_unit: also count every unit in an array (small sweeps); the chained walk below already proves exact coverage */
static int check(int tiles, int nkt, int G, int per_unit)
{
    const int U = tiles * nkt;
    int g = 0;
    static int first_slot[MAX_TILES], nseg[MAX_TILES], next_kt[MAX_TILES];
    static unsigned char slot_used[MAX_G + MAX_TILES], unit_buf[MAX_UNITS];
    unsigned char* unit_seen = per_unit ? unit_buf : NULL;
    if (tiles > MAX_TILES || G > MAX_G || (per_unit && U > MAX_UNITS)) FAIL("sweep larger than the checker's buffers");
    memset(nseg, 0, sizeof(int) * (size_t) tiles);
    memset(next_kt, 0, sizeof(int) * (size_t) tiles);
    memset(slot_used, 0, (size_t) (G + tiles));
    if (unit_seen) memset(unit_seen, 0, (size_t) U);
    int covered = 0, last_slot = -1, owners = 0;
    for (g = 0; g < G; ++g) {
        int u = tn_even_unit0(g, G, U);
        const int u1 = tn_even_unit0(g + 1, G, U), rank = tn_even_rank(g, G, U);
        if (u != covered) FAIL("workgroup ranges do not chain");
        if (u1 < u || u1 > U) FAIL("range out of order");
        if (rank != owners) FAIL("rank is not the number of non-empty workgroups before g");
        if (u1 > u) ++owners;
        while (u < u1) {                                      /* an empty workgroup never gets here: it owns no slot */
            const tn_even_seg s = tn_even_seg_at(u, u1, nkt, rank);
            if (s.nkt < 1) FAIL("empty segment");
            if (s.tile < 0 || s.tile >= tiles || s.tile * nkt + s.kt0 != u) FAIL("segment does not start at its unit");
            if (s.kt0 + s.nkt > nkt) FAIL("segment crosses a tile");
            if (u + s.nkt > u1) FAIL("segment leaves the workgroup's range");
            if (s.slot < 0 || s.slot >= G + tiles) FAIL("slot out of range");
            if (slot_used[s.slot]) FAIL("slot used twice");
            slot_used[s.slot] = 1;
            if (s.slot <= last_slot) FAIL("slots not ascending in walk order");
            last_slot = s.slot;
            if (nseg[s.tile] == 0) first_slot[s.tile] = s.slot;
            else if (s.slot != first_slot[s.tile] + nseg[s.tile]) FAIL("a tile's slots are not consecutive");
            if (s.kt0 != next_kt[s.tile]) FAIL("a tile's segments are not ascending and gap-free in k");
            next_kt[s.tile] = s.kt0 + s.nkt;
            ++nseg[s.tile];
            if (tn_even_owner(u, G, U) != g || tn_even_owner(u + s.nkt - 1, G, U) != g) FAIL("owner() disagrees");
            if (unit_seen)
                for (int k = 0; k < s.nkt; ++k) {
                    if (unit_seen[u + k]) FAIL("unit covered twice");
                    unit_seen[u + k] = 1;
                }
            u += s.nkt;
        }
        covered = u1;
    }
    g = -1;
    if (covered != U) FAIL("units left over");
    for (int t = 0; t < tiles; ++t) {
        int f, c;
        tn_even_tile_slots(t, G, tiles, nkt, &f, &c);
        if (next_kt[t] != nkt) FAIL("tile not covered in k");
        if (f != first_slot[t] || c != nseg[t]) FAIL("tn_even_tile_slots() disagrees with the segments");
    }
    if (unit_seen)
        for (int u = 0; u < U; ++u)
            if (!unit_seen[u]) FAIL("unit never covered");
    int used = 0, total = 0;
    for (int s = 0; s < G + tiles; ++s) used += slot_used[s];
    for (int t = 0; t < tiles; ++t) total += nseg[t];
    if (used != total) FAIL("slot count");
    return 0;
}

int main(void)
{
    long triples = 0;
    for (int tiles = 1; tiles <= 40; ++tiles)
        for (int nkt = 1; nkt <= 40; ++nkt)
            for (int G = 1; G <= 96; ++G, ++triples)
                if (check(tiles, nkt, G, 1)) return 1;
    /* the wide update's own range at 16384^2, nb 256: 50 ... 248 tiles, up to 1024 k-tiles, the 224- and 256-CU streams */
    for (int tiles = 50; tiles <= 248; ++tiles)
        for (int nkt = 1; nkt <= 1024; ++nkt)
            for (int G = 448; G <= 512; G += 64, ++triples)
                if (check(tiles, nkt, G, 0)) return 1;
    printf("tn_even_check ok %ld\n", triples);
    return 0;
}
