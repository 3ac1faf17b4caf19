/* hap_junctions_check.c — c3r_hap_junction_counts / c3r_get_hap_junctions / c3r_set_hap_junction_direct through the C ABI alone: the arguments
 * the calls must refuse, the getter before anything was counted, the empty result without reads, and that the context is usable afterwards.  No
 * reads are loaded, so no kernel runs (the context itself needs a device).  Built as plain C against include/c3r.h and libc3r.so:
 *   cc -std=c11 -Wall -Iinclude tests/c/hap_junctions_check.c -Lclair3_rna_amd -lc3r -Wl,-rpath,<dir of libc3r.so> -o hap_junctions_check
 * Prints "hap_junctions_check: ok" and exits 0, or says what differed and exits 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3r.h"

static int failures = 0;
static c3r_ctx *ctx;

static void expect(const char *name, int rc, int want, const char *key) {
    const char *msg = c3r_last_error(ctx);
    if (rc != want || (want != C3R_OK && key && (!msg || !strstr(msg, key)))) {
        printf("%s: returned %d (want %d), message \"%s\" (want \"%s\")\n", name, rc, want, msg ? msg : "", key ? key : "");
        ++failures;
    }
}

int main(void) {
    if (sizeof(c3r_hap_junction_t) != 24 || sizeof(c3r_hap_junction_row_t) != 12) { printf("layout: %zu and %zu bytes\n", sizeof(c3r_hap_junction_t), sizeof(c3r_hap_junction_row_t)); return 1; }
    int rc = c3r_create(0, NULL, &ctx);
    if (rc != C3R_OK) { printf("c3r_create: %d\n", rc); return 1; }
    c3r_hap_junction_t j[2];
    c3r_hap_junction_row_t r[2];
    int64_t nj = -1, nr = -1;

    /* nothing counted yet */
    expect("getter before a count", c3r_get_hap_junctions(ctx, j, 2, r, 2), C3R_EINVAL, "nothing has been counted");

    /* arguments that are none */
    expect("no context", c3r_hap_junction_counts(NULL, 0, &nj, &nr), C3R_EINVAL, NULL);
    expect("no n_junctions", c3r_hap_junction_counts(ctx, 0, NULL, &nr), C3R_EINVAL, NULL);
    expect("no n_rows", c3r_hap_junction_counts(ctx, 0, &nj, NULL), C3R_EINVAL, NULL);
    expect("negative slots_hint", c3r_hap_junction_counts(ctx, -1, &nj, &nr), C3R_EINVAL, "negative");
    expect("getter after the refusals", c3r_get_hap_junctions(ctx, j, 2, r, 2), C3R_EINVAL, "nothing has been counted");

    /* no reads loaded, no phase table: both counts 0, and that is a result */
    for (int direct = 0; direct <= 1; ++direct) {
        expect("set the variant", c3r_set_hap_junction_direct(ctx, direct), C3R_OK, NULL);
        for (int64_t hint = 0; hint <= 4096; hint = hint ? hint * 64 : 1) {
            nj = nr = -1;
            expect("no reads", c3r_hap_junction_counts(ctx, hint, &nj, &nr), C3R_OK, NULL);
            if (nj != 0 || nr != 0) { printf("no reads: %lld junctions, %lld rows\n", (long long)nj, (long long)nr); ++failures; }
        }
        expect("empty result", c3r_get_hap_junctions(ctx, NULL, 0, NULL, 0), C3R_OK, NULL);
        expect("empty result into arrays", c3r_get_hap_junctions(ctx, j, 2, r, 2), C3R_OK, NULL);
        expect("negative capacity", c3r_get_hap_junctions(ctx, j, -1, r, 2), C3R_EINVAL, NULL);
        expect("negative row capacity", c3r_get_hap_junctions(ctx, j, 2, r, -1), C3R_EINVAL, NULL);
    }
    expect("variant 2", c3r_set_hap_junction_direct(ctx, 2), C3R_EINVAL, "neither 0 nor 1");
    expect("variant -1", c3r_set_hap_junction_direct(ctx, -1), C3R_EINVAL, "neither 0 nor 1");
    expect("no context for the variant", c3r_set_hap_junction_direct(NULL, 0), C3R_EINVAL, NULL);
    expect("no context for the getter", c3r_get_hap_junctions(NULL, j, 2, r, 2), C3R_EINVAL, NULL);

    /* with a phase table and still no reads: the same */
    c3r_phase_site_t p;
    memset(&p, 0, sizeof p);
    p.pos = 5; p.ps = 1; p.ref = 1; p.alt = 2;
    expect("set a table", c3r_set_phase_sites(ctx, &p, 1), C3R_OK, NULL);
    expect("no reads under a table", c3r_hap_junction_counts(ctx, 0, &nj, &nr), C3R_OK, NULL);
    if (nj != 0 || nr != 0) { printf("no reads under a table: %lld junctions, %lld rows\n", (long long)nj, (long long)nr); ++failures; }

    /* a load — of no reads — forgets the result */
    uint32_t none = 0;
    uint8_t seq = 0;
    c3r_read_t read;
    memset(&read, 0, sizeof read);
    expect("load no reads", c3r_load_reads(ctx, &read, 0, &none, 0, &seq, 0), C3R_OK, NULL);
    expect("getter after a load", c3r_get_hap_junctions(ctx, j, 2, r, 2), C3R_EINVAL, "nothing has been counted");
    expect("count again", c3r_hap_junction_counts(ctx, 0, &nj, &nr), C3R_OK, NULL);
    expect("getter after the count", c3r_get_hap_junctions(ctx, j, 2, r, 2), C3R_OK, NULL);

    /* the context is usable afterwards: the table is still set */
    c3r_haplotag_stats_t st;
    expect("haplotags after the refusals", c3r_get_haplotags(ctx, NULL, 0, &st), C3R_OK, NULL);

    c3r_destroy(ctx);
    if (failures) { printf("hap_junctions_check: %d failure(s)\n", failures); return 1; }
    printf("hap_junctions_check: ok\n");
    return 0;
}
