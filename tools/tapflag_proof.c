// tapflag_proof.c -- host-side proof of the NARROW brick kernels' tap-cell flags (csrc/dr_brick_common.h, "tap-cell flags"):
// whether a +-delta tap sits in the centre tap's cell is read from the fractions,
//     cell(p + delta) == cell(p)  <=>  fr(p + delta) >= fr(p)
//     cell(p - delta) == cell(p)  <=>  fr(p - delta) <= fr(p)
// and a tap is never more than one cell away. axis_coord (csrc/dr_brick.h) is restated here in C, operation for operation:
// fmaf, fmaxf, fminf, one multiply, truncation, q - floorf(q) (what v_fract_f32 returns for q >= 0). Build with contraction
// off, as the kernels are:
//     cc -O2 -ffp-contract=off -fopenmp -o tapflag_proof tools/tapflag_proof.c -lm       (-fopenmp is optional)
// Usage:
//     tapflag_proof full              every float position in [-1 - 2 delta, 1 + 2 delta] at the ten edges below, then the edge scan
//     tapflag_proof reduced [N]       all floats within 64 ulps of every position where q, q+ or q- is an integer, the clamp
//                                     points +-1 and +-(1 +- delta) likewise, and N (default 10^7) random positions per edge
//     tapflag_proof scan              only the edge scan: the smallest edge (2 .. 4100) at which an equivalence fails
//     tapflag_proof edge E...         the reduced set without the random positions at the given edges (2001 has counter-examples:
//                                     the check is not vacuous)
// Exit status 0: no counter-example at any of the ten edges and none in the scan at or below 991 (taps_narrow's limit).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const float DELTA = 1e-3f;
static const int EDGES[] = {2, 3, 13, 14, 25, 96, 256, 512, 990, 991};
enum { NEDGES = sizeof(EDGES) / sizeof(EDGES[0]), NARROW_MAX_EDGE = 991 };

static inline float edge_scale(int edge) { return (float)((double)edge - 1.0 - 1e-4); }   // dr_tile.h: VolView's scx
static inline float axis_q(float pos, float sc) { return fminf(1.0f, fmaxf(0.0f, fmaf(0.5f, pos, 0.5f))) * sc; }
static inline void axis_coord(float pos, float sc, int *cell, float *fr) {
    const float q = axis_q(pos, sc);
    *fr = q - floorf(q);
    *cell = (int)q;
}

typedef struct { uint64_t checked, failed; float pos; int edge, kind; } Tally;
static const char *KIND[] = {"", "cell(p+d) == cell(p) <=> fr+ >= fr", "cell(p-d) == cell(p) <=> fr- <= fr", "|cell(p+-d) - cell(p)| <= 1"};

// returns 0, or which statement fails at this position
static inline int check_pos(float p, float sc) {
    int c0, cp, cm;
    float f0, fp, fm;
    axis_coord(p, sc, &c0, &f0);
    axis_coord(p + DELTA, sc, &cp, &fp);
    axis_coord(p - DELTA, sc, &cm, &fm);
    if ((cp == c0) != (fp >= f0)) return 1;
    if ((cm == c0) != (fm <= f0)) return 2;
    if (cp - c0 > 1 || cp - c0 < -1 || cm - c0 > 1 || cm - c0 < -1) return 3;
    return 0;
}
static inline void tally(Tally *t, float p, float sc, int edge) {
    const int k = check_pos(p, sc);
    t->checked++;
    if (k) { if (!t->failed) { t->pos = p; t->edge = edge; t->kind = k; } t->failed++; }
}

// floats as ordered integers: key(x) is monotone in x
static inline int64_t f2key(float x) { int32_t i; memcpy(&i, &x, 4); return i >= 0 ? (int64_t)i : -(int64_t)(i & 0x7fffffff); }
static inline float key2f(int64_t k) { int32_t i = k >= 0 ? (int32_t)k : (int32_t)((uint32_t)(-k) | 0x80000000u); float x; memcpy(&x, &i, 4); return x; }

static void window(Tally *t, float centre, int ulps, float sc, int edge) {
    const int64_t k0 = f2key(centre);
    for (int64_t k = k0 - ulps; k <= k0 + ulps; ++k) tally(t, key2f(k), sc, edge);
}

// every position near which one of q, q+, q- crosses an integer, and the clamp points
static void critical(Tally *t, int edge, int ulps) {
    const float sc = edge_scale(edge);
    for (int n = 0; n <= edge; ++n) {
        const float p = (float)(2.0 * (double)n / (double)sc - 1.0);   // q(p) = n
        window(t, p, ulps, sc, edge);
        window(t, p - DELTA, ulps, sc, edge);                          // q+ = n
        window(t, p + DELTA, ulps, sc, edge);                          // q- = n
    }
    const float cl[] = {1.0f, -1.0f, 1.0f + DELTA, 1.0f - DELTA, -1.0f + DELTA, -1.0f - DELTA};
    for (int i = 0; i < 6; ++i) window(t, cl[i], ulps, sc, edge);
}

static uint64_t rng_next(uint64_t *s) { *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17; return *s; }
static void randoms(Tally *t, int edge, long n) {
    const float sc = edge_scale(edge);
    uint64_t s = 0x9e3779b97f4a7c15ull ^ (uint64_t)edge;
    const double lo = -1.0 - 2.0 * DELTA, span = 2.0 + 4.0 * DELTA;
    for (long i = 0; i < n; ++i) tally(t, (float)(lo + span * ((double)(rng_next(&s) >> 11) * (1.0 / 9007199254740992.0))), sc, edge);
}

static void merge(Tally *a, const Tally *b) {
    if (!a->failed && b->failed) { a->pos = b->pos; a->edge = b->edge; a->kind = b->kind; }
    a->checked += b->checked; a->failed += b->failed;
}

static void exhaustive(Tally *t, int edge) {
    const float sc = edge_scale(edge);
    const int64_t k0 = f2key(-1.0f - 2.0f * DELTA), k1 = f2key(1.0f + 2.0f * DELTA);
    enum { CH = 1 << 20 };
    const int64_t nch = (k1 - k0 + CH) / CH;
    uint64_t checked = 0, failed = 0;
    int64_t first_bad = INT64_MAX;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : checked, failed) reduction(min : first_bad)
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t a = k0 + c * CH, b = a + CH - 1 < k1 ? a + CH - 1 : k1;
        for (int64_t k = a; k <= b; ++k) {
            ++checked;
            if (check_pos(key2f(k), sc)) { ++failed; if (k < first_bad) first_bad = k; }
        }
    }
    Tally u = {checked, failed, 0.0f, edge, 0};
    if (failed) { u.pos = key2f(first_bad); u.kind = check_pos(u.pos, sc); }
    merge(t, &u);
}

static void report(const char *what, int edge, const Tally *t) {
    printf("%-10s edge %4d  sc %.6f  delta' %.6f voxels  positions %12llu  counter-examples %llu", what, edge, (double)edge_scale(edge),
           (double)(0.5f * DELTA * edge_scale(edge)), (unsigned long long)t->checked, (unsigned long long)t->failed);
    if (t->failed) printf("  first: p = %.9g (%a): %s", (double)t->pos, (double)t->pos, KIND[t->kind]);
    printf("\n");
}

// smallest edge at which one of the statements fails on the critical positions (0: none up to `upto`)
static int edge_scan(int upto) {
    int first = 0;
    for (int edge = 2; edge <= upto && !first; ++edge) {
        Tally t; memset(&t, 0, sizeof t);
        critical(&t, edge, 64);
        if (t.failed) { first = edge; report("scan", edge, &t); }
    }
    if (first) printf("scan: the equivalences first fail at edge %d (taps_narrow's limit: %d)\n", first, NARROW_MAX_EDGE);
    else printf("scan: no counter-example at any edge 2 .. %d\n", upto);
    return first;
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "reduced";
    const long nrand = argc > 2 ? atol(argv[2]) : 10000000L;
    int bad = 0;
    if (!strcmp(mode, "full") || !strcmp(mode, "reduced")) {
        const int full = !strcmp(mode, "full");
        for (int i = 0; i < NEDGES; ++i) {
            Tally t; memset(&t, 0, sizeof t);
            if (full) exhaustive(&t, EDGES[i]);
            else { critical(&t, EDGES[i], 64); randoms(&t, EDGES[i], nrand); }
            report(mode, EDGES[i], &t);
            bad |= t.failed != 0;
        }
    } else if (!strcmp(mode, "edge")) {
        for (int i = 2; i < argc; ++i) {
            const int edge = atoi(argv[i]);
            Tally t; memset(&t, 0, sizeof t);
            if (edge >= 2) { critical(&t, edge, 64); report("edge", edge, &t); }
            bad |= t.failed != 0 && edge <= NARROW_MAX_EDGE;
        }
    } else if (strcmp(mode, "scan")) {
        fprintf(stderr, "usage: tapflag_proof full | reduced [N] | scan | edge E...\n");
        return 2;
    }
    if (!strcmp(mode, "full") || !strcmp(mode, "scan")) {
        const int first = edge_scan(4100);
        bad |= first != 0 && first <= NARROW_MAX_EDGE;
    }
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
