/* hap_regions_check.c — c3r_hap_region_counts through the C ABI alone: every table the call must refuse, with the return code and the region
 * or row c3r_last_error names, the refusal without a phase table, and that the context is usable afterwards.  All inputs are host arrays made
 * here; no reads are loaded, so no kernel runs (the context itself needs a device).  Built as plain C against include/c3r.h and libc3r.so:
 *   cc -std=c11 -Wall -Iinclude tests/c/hap_regions_check.c -Lclair3_rna_amd -lc3r -Wl,-rpath,<dir of libc3r.so> -o hap_regions_check
 * Prints "hap_regions_check: ok" and exits 0, or says what differed and exits 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3r.h"

static int failures = 0;
static c3r_ctx *ctx;

static c3r_hap_region_t region(int32_t start, int32_t end, int32_t row_off, uint8_t strand) {
    c3r_hap_region_t r;
    memset(&r, 0, sizeof r);
    r.start = start; r.end = end; r.row_off = row_off; r.strand = strand;
    return r;
}

/* the good table: four regions — two equal, one nested — over five rows */
#define N 4
#define N_ROWS 5
static void good(c3r_hap_region_t *t, int32_t *ps) {
    t[0] = region(10, 100, 0, 0);       /* rows 0, 1: sets 3, 9 */
    t[1] = region(10, 100, 2, 1);       /* row 2: set 3 */
    t[2] = region(20, 30, 3, 2);        /* no row */
    t[3] = region(200, 201, 3, 0);      /* rows 3, 4: sets 0, 7 */
    ps[0] = 3; ps[1] = 9; ps[2] = 3; ps[3] = 0; ps[4] = 7;
}

static void expect(const char *name, int rc, int want, const char *key) {
    const char *msg = c3r_last_error(ctx);
    if (rc != want || (want != C3R_OK && key && (!msg || !strstr(msg, key)))) {
        printf("%s: returned %d (want %d), message \"%s\" (want \"%s\")\n", name, rc, want, msg ? msg : "", key ? key : "");
        ++failures;
    }
}

int main(void) {
    int rc = c3r_create(0, NULL, &ctx);
    if (rc != C3R_OK) { printf("c3r_create: %d\n", rc); return 1; }
    c3r_hap_region_t t[N];
    int32_t ps[N_ROWS];
    uint32_t rc_out[2 * N], wc_out[2 * N_ROWS];

    /* no phase table: refused with hap_count_table's message, whatever n is */
    good(t, ps);
    expect("no table", c3r_hap_region_counts(ctx, t, N, ps, N_ROWS, 0, rc_out, wc_out), C3R_EINVAL, "no phase sites are set");
    expect("no table, n = 0", c3r_hap_region_counts(ctx, NULL, 0, NULL, 0, 0, NULL, NULL), C3R_EINVAL, "no phase sites are set");

    c3r_phase_site_t p;
    memset(&p, 0, sizeof p);
    p.pos = 5; p.ps = 1; p.ref = 1; p.alt = 2;
    expect("set a table", c3r_set_phase_sites(ctx, &p, 1), C3R_OK, NULL);

    /* the good table with no reads loaded: OK, every count 0 */
    memset(rc_out, 0xff, sizeof rc_out);
    memset(wc_out, 0xff, sizeof wc_out);
    expect("good table", c3r_hap_region_counts(ctx, t, N, ps, N_ROWS, 2, rc_out, wc_out), C3R_OK, NULL);
    for (int k = 0; k < 2 * N; ++k) if (rc_out[k]) { printf("good table: region_counts[%d] = %u without reads\n", k, rc_out[k]); ++failures; break; }
    for (int k = 0; k < 2 * N_ROWS; ++k) if (wc_out[k]) { printf("good table: row_counts[%d] = %u without reads\n", k, wc_out[k]); ++failures; break; }
    expect("n = 0", c3r_hap_region_counts(ctx, NULL, 0, NULL, 0, 0, NULL, NULL), C3R_OK, NULL);
    expect("regions without rows", c3r_hap_region_counts(ctx, t, 1, NULL, 0, 0, rc_out, NULL), C3R_OK, NULL);

#define BAD(name, key, stranded, change) do { good(t, ps); change; \
        expect(name, c3r_hap_region_counts(ctx, t, N, ps, N_ROWS, stranded, rc_out, wc_out), C3R_EINVAL, key); } while (0)
    BAD("unsorted by start", "region 3:", 0, t[3].start = 15);
    BAD("unsorted by end", "region 1:", 0, t[1].end = 99);
    BAD("start == end", "region 2:", 0, t[2].end = 20);
    BAD("start > end", "region 0:", 0, t[0].end = 5);
    BAD("negative start", "region 0:", 0, t[0].start = -1);
    BAD("row_off[0] != 0", "region 0:", 0, t[0].row_off = 1);
    BAD("row_off decreases", "region 2:", 0, t[2].row_off = 1);
    BAD("row_off past n_rows", "region 3:", 0, t[3].row_off = 6);
    BAD("negative row_off", "region 1:", 0, t[1].row_off = -1);
    BAD("row_ps not increasing", "row 1 (region 0):", 0, ps[1] = 3);
    BAD("row_ps decreasing", "row 4 (region 3):", 0, (ps[3] = 8));
    BAD("negative ps", "row 2 (region 1):", 0, ps[2] = -1);
    BAD("strand above 2", "region 2:", 0, t[2].strand = 3);
    BAD("reserved byte", "region 1:", 0, t[1].reserved[2] = 1);
    BAD("stranded 3", "stranded 3", 3, (void)0);
    BAD("stranded -1", "stranded -1", -1, (void)0);
    /* the first bad region is the one named */
    BAD("two bad regions", "region 1:", 0, (t[1].strand = 9, t[3].end = 0));
#undef BAD
    /* sets may repeat across regions and need not increase from one region to the next */
    good(t, ps);
    expect("equal sets in two regions", c3r_hap_region_counts(ctx, t, N, ps, N_ROWS, 0, rc_out, wc_out), C3R_OK, NULL);

    /* arguments that are no table at all */
    expect("no context", c3r_hap_region_counts(NULL, t, N, ps, N_ROWS, 0, rc_out, wc_out), C3R_EINVAL, NULL);
    expect("negative n", c3r_hap_region_counts(ctx, t, -1, ps, N_ROWS, 0, rc_out, wc_out), C3R_EINVAL, NULL);
    expect("negative n_rows", c3r_hap_region_counts(ctx, t, N, ps, -1, 0, rc_out, wc_out), C3R_EINVAL, NULL);
    expect("no regions", c3r_hap_region_counts(ctx, NULL, N, ps, N_ROWS, 0, rc_out, wc_out), C3R_EINVAL, NULL);
    expect("no row_ps", c3r_hap_region_counts(ctx, t, N, NULL, N_ROWS, 0, rc_out, wc_out), C3R_EINVAL, NULL);
    expect("no region_counts", c3r_hap_region_counts(ctx, t, N, ps, N_ROWS, 0, NULL, wc_out), C3R_EINVAL, NULL);
    expect("no row_counts", c3r_hap_region_counts(ctx, t, N, ps, N_ROWS, 0, rc_out, NULL), C3R_EINVAL, NULL);
    expect("rows without a region", c3r_hap_region_counts(ctx, NULL, 0, ps, N_ROWS, 0, NULL, wc_out), C3R_EINVAL, NULL);

    /* the bound: one region over MAX_BACK + 1 short ones is refused, naming the first region that lies too far behind it; over MAX_BACK it passes */
    {
        const int n = C3R_HAP_REGION_MAX_BACK + 2;
        c3r_hap_region_t *big = (c3r_hap_region_t *)malloc(sizeof(c3r_hap_region_t) * (size_t)n);
        uint32_t *out = (uint32_t *)malloc(8 * (size_t)n);
        char key[64];
        big[0] = region(0, 10 * n, 0, 0);
        for (int k = 1; k < n; ++k) big[k] = region(10 * k, 10 * k + 5, 0, 0);
        snprintf(key, sizeof key, "region %d:", C3R_HAP_REGION_MAX_BACK + 1);
        expect("over the bound", c3r_hap_region_counts(ctx, big, n, NULL, 0, 0, out, NULL), C3R_EINVAL, key);
        expect("over the bound: the advice", C3R_EINVAL, C3R_EINVAL, "separate calls");
        expect("over the bound: the bound's name", C3R_EINVAL, C3R_EINVAL, "C3R_HAP_REGION_MAX_BACK");
        expect("at the bound", c3r_hap_region_counts(ctx, big, n - 1, NULL, 0, 0, out, NULL), C3R_OK, NULL);
        /* the same regions without the long one: nothing is open behind any of them */
        expect("without the long region", c3r_hap_region_counts(ctx, big + 1, n - 1, NULL, 0, 0, out, NULL), C3R_OK, NULL);
        free(big);
        free(out);
    }

    /* the context is usable afterwards: the table is still set and the call still works */
    c3r_haplotag_stats_t st;
    expect("haplotags after the refusals", c3r_get_haplotags(ctx, NULL, 0, &st), C3R_OK, NULL);
    good(t, ps);
    expect("good table after the refusals", c3r_hap_region_counts(ctx, t, N, ps, N_ROWS, 1, rc_out, wc_out), C3R_OK, NULL);

    c3r_destroy(ctx);
    if (failures) { printf("hap_regions_check: %d failure(s)\n", failures); return 1; }
    printf("hap_regions_check: ok\n");
    return 0;
}
