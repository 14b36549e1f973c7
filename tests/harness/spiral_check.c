/*
 * spiral_check.c — JM's spiral order as csrc/jmh_spiral.h states it (the text ordtab_fill of
 * csrc/jmhip_abi.hip and subpel_wave of csrc/jmh_analyse.hip compile) on the CPU (TEST
 * INFRASTRUCTURE).
 *
 * The spiral is generated here by the nested loops of Init_Motion_Search_Module (docs/JM_SEMANTICS.md
 * item 5), not by the closed form: index 0 is (0,0); for l = 1 .. max(1, sr): for i = -l+1 .. l-1 the
 * pair (i, -l), (i, +l); then for i = -l .. l the pair (-l, i), (+l, i).  For every sr in 1..32 and
 * every index n < (2 sr + 1)^2:
 *   (a) jms_decode(n) is the loops' position, and jms_index(position) is n;
 *   (b) jms_ring(n) is max(|x|, |y|), and jms_ring_fix(n, l) repairs the candidates l - 1, l, l + 1 (what
 *       the device's square root may hand it, whatever its rounding) to that ring;
 *   (c) jms_ordtab_fill's three tables (order keys of the analysis threads, index -> position, raster
 *       position -> index) are bit for bit those of the function it replaced, kept below as
 *       old_ordtab_fill with its own spiral index.  Both tables are malloc blocks of exactly their
 *       words, so a write outside them is an ASan error.
 *
 * Exit 0: everything equal.  Built with -fsanitize=address,undefined (tests/harness/spiral.mk).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../h264-jm-commentary_amd/csrc/jmh_spiral.h"

#define SR_MAX 32
#define NPK 10      /* csrc/jmh_device.h: positions per analysis thread */
#define NTA 512     /*                    threads per analysis workgroup */
#define NPK2 ((NPK + 1) / 2)
#define ORDTAB_SPOS (NPK2 * NTA)

static long s_idx, s_bad;

static void bad(const char *what, int sr, int n) {
    if (s_bad++ < 20) fprintf(stderr, "spiral check: %s differs at sr %d index %d\n", what, sr, n);
}

/* Init_Motion_Search_Module's loops: n positions written, sx / sy hold (2 sr + 1)^2 entries */
static int jm_spiral(int sr, int *sx, int *sy) {
    int k = 1, l, i;
    const int lmax = sr > 1 ? sr : 1;
    sx[0] = sy[0] = 0;
    for (l = 1; l <= lmax; l++) {
        for (i = -l + 1; i < l; i++) {
            sx[k] = i; sy[k++] = -l;
            sx[k] = i; sy[k++] = l;
        }
        for (i = -l; i <= l; i++) {
            sx[k] = -l; sy[k++] = i;
            sx[k] = l; sy[k++] = i;
        }
    }
    return k;
}

/* the table fill before jmh_spiral.h, with its own position -> index */
static int old_spiral_index(int x, int y) {
    const int ax = x < 0 ? -x : x, ay = y < 0 ? -y : y, l = ax > ay ? ax : ay;
    if (l == 0) return 0;
    const int base = (2 * l - 1) * (2 * l - 1);
    if (ay == l && ax < l) return base + 2 * (x + l - 1) + (y > 0);
    return base + 2 * (2 * l - 1) + 2 * (y + l) + (x > 0);
}
static void old_ordtab_fill(uint32_t *tab, int sr) {
    const int side = 2 * sr + 1, nstrips = (side + NPK - 1) / NPK;
    int x, y, t, k;
    for (y = -sr; y <= sr; y++)
        for (x = -sr; x <= sr; x++) {
            tab[(size_t)ORDTAB_SPOS + old_spiral_index(x, y)] = ((uint32_t)x & 0xFFFFu) | (uint32_t)y << 16;
            tab[(size_t)ORDTAB_SPOS + (size_t)side * side + (size_t)(y + sr) * side + x + sr] = (uint32_t)old_spiral_index(x, y);
        }
    for (t = 0; t < NTA; t++) {
        const int sact = t < side * nstrips;
        const int dx = sact ? t % side : 0, dy0 = sact ? (t / side) * NPK : 0;
        for (k = 0; k < NPK; k++) {
            const int dy = dy0 + k;
            const uint32_t o = (!sact || dy >= side) ? 0xFFFFu : (uint32_t)(old_spiral_index(dx - sr, dy - sr) + 1);
            tab[(size_t)(k >> 1) * NTA + t] |= o << (16 * (k & 1));
        }
    }
}

int main(void) {
    int sr, tables = 0;
    for (sr = 1; sr <= SR_MAX; sr++) {
        const int side = 2 * sr + 1, np = side * side;
        int *sx = malloc(sizeof(int) * np), *sy = malloc(sizeof(int) * np), n;
        if (!sx || !sy) return 2;
        if (jm_spiral(sr, sx, sy) != np) { bad("the loops' count", sr, np); }
        for (n = 0; n < np; n++) {
            int x = 99, y = 99, l, ring, c;
            jms_decode(n, &x, &y);
            if (x != sx[n] || y != sy[n]) bad("jms_decode", sr, n);
            if (jms_index(sx[n], sy[n]) != n) bad("jms_index", sr, n);
            ring = abs(sx[n]) > abs(sy[n]) ? abs(sx[n]) : abs(sy[n]);
            l = jms_ring(n);
            if (l != ring) bad("jms_ring", sr, n);
            for (c = ring - 1; c <= ring + 1; c++)
                if (c >= 0 && jms_ring_fix(n, c) != ring) bad("jms_ring_fix", sr, n);
            x = y = 99;
            jms_ring_pos(n, ring, &x, &y);
            if (x != sx[n] || y != sy[n]) bad("jms_ring_pos", sr, n);
            s_idx++;
        }
        free(sx); free(sy);
        {   /* (c) the tables */
            const size_t len = (size_t)ORDTAB_SPOS + (size_t)2 * np;
            uint32_t *a = calloc(len, sizeof(uint32_t)), *b = calloc(len, sizeof(uint32_t));
            size_t i;
            if (!a || !b) return 2;
            if (jms_ordtab_len(sr, NPK, NTA) != len) bad("jms_ordtab_len", sr, 0);
            old_ordtab_fill(a, sr);
            jms_ordtab_fill(b, sr, NPK, NTA);
            for (i = 0; i < len; i++)
                if (a[i] != b[i]) { bad("jms_ordtab_fill", sr, (int)i); break; }
            tables += memcmp(a, b, len * sizeof(uint32_t)) == 0;
            free(a); free(b);
        }
    }
    printf("spiral check: %d ranges, %ld indices, %d tables equal, %ld differ\n", SR_MAX, s_idx, tables, s_bad);
    return s_bad ? 1 : 0;
}
