/* phase_alleles_check.c — c3r_set_phase_alleles through the C ABI alone: every table the call must refuse, with the return code and the
 * index c3r_last_error names, and that a refused table leaves the one set before in force.  All inputs are host arrays made here; no reads
 * are loaded, so no kernel runs (the context itself needs a device).  Built as plain C against include/c3r.h and libc3r.so:
 *   cc -std=c11 -Wall -Iinclude tests/c/phase_alleles_check.c -Lclair3_rna_amd -lc3r -Wl,-rpath,<dir of libc3r.so> -o phase_alleles_check
 * Prints "phase_alleles_check: ok" and exits 0, or says what differed and exits 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3r.h"

static int failures = 0;
static c3r_ctx *ctx;

static c3r_hap_site_t snv(int32_t pos, int32_t ps, uint8_t ref, uint8_t alt) {
    c3r_hap_site_t s;
    memset(&s, 0, sizeof s);
    s.pos = pos; s.ps = ps; s.base_matters = 1;
    s.a.base = ref; s.b.base = alt;
    return s;
}

static c3r_hap_site_t indel(int32_t pos, int32_t ps, uint8_t base, uint8_t kind, uint16_t len, uint32_t off) {
    c3r_hap_site_t s;
    memset(&s, 0, sizeof s);
    s.pos = pos; s.ps = ps; s.event_matters = 1;
    s.a.base = base; s.b.base = base; s.b.kind = kind; s.b.len = len; s.b.ins_off = off;
    return s;
}

/* the good table: an SNV, an insertion of the pool's bases 0 .. 2 (A C G), a deletion of 2 */
static const uint8_t POOL[2] = {0x12, 0x40};
static void good(c3r_hap_site_t *t, uint8_t *h1) {
    t[0] = snv(10, 1, 1, 2);
    t[1] = indel(20, 1, 4, C3R_HAP_EV_INS, 3, 0);
    t[2] = indel(30, 2, 8, C3R_HAP_EV_DEL, 2, 0);
    h1[0] = 0; h1[1] = 1; h1[2] = 0;
}

static void expect(const char *name, int rc, int want, int index) {
    char key[64];
    snprintf(key, sizeof key, "phase allele site %d:", index);
    const char *msg = c3r_last_error(ctx);
    if (rc != want || (want != C3R_OK && index >= 0 && (!msg || !strstr(msg, key)))) {
        printf("%s: returned %d (want %d), message \"%s\" (want \"%s\")\n", name, rc, want, msg ? msg : "", index >= 0 ? key : "");
        ++failures;
    }
}

/* the table set before is still there: c3r_get_haplotags succeeds only while a table is set */
static void still_set(const char *name, int want_set) {
    c3r_haplotag_stats_t st;
    const int rc = c3r_get_haplotags(ctx, NULL, 0, &st);
    if ((rc == C3R_OK) != (want_set != 0)) { printf("%s: a table is %sset afterwards\n", name, rc == C3R_OK ? "" : "not "); ++failures; }
}

int main(void) {
    int rc = c3r_create(0, NULL, &ctx);
    if (rc != C3R_OK) { printf("c3r_create: %d\n", rc); return 1; }
    c3r_hap_site_t t[3];
    uint8_t h1[3], pool[2];
    memcpy(pool, POOL, 2);

    still_set("fresh context", 0);
    good(t, h1);
    expect("good table", c3r_set_phase_alleles(ctx, t, h1, 3, pool, 3), C3R_OK, -1);
    still_set("good table", 1);

#define BAD(name, index, change) do { good(t, h1); memcpy(pool, POOL, 2); change; \
        expect(name, c3r_set_phase_alleles(ctx, t, h1, 3, pool, 3), C3R_EINVAL, index); still_set(name, 1); } while (0)
    BAD("unsorted", 2, t[2].pos = 15);
    BAD("repeated", 1, t[1].pos = 10);
    BAD("pos below 1", 0, t[0].pos = 0);
    BAD("negative ps", 1, t[1].ps = -1);
    BAD("flag above 1", 2, t[2].event_matters = 2);
    BAD("bad base", 0, t[0].b.base = 3);
    BAD("unknown kind", 1, t[1].b.kind = 3);
    BAD("insertion of length 0", 1, t[1].b.len = 0);
    BAD("length without an event", 0, t[0].a.len = 1);
    BAD("insertion past the pool", 1, t[1].b.ins_off = 1);
    BAD("bad base in the pool", 1, pool[0] = 0x1f);
    BAD("equal alleles", 2, (t[2].a.kind = C3R_HAP_EV_DEL, t[2].a.len = 2));
    BAD("h1 above 1", 1, h1[1] = 2);
    BAD("h1 above 1 on the last site", 2, h1[2] = 255);
    /* the first bad index is the one named */
    BAD("two bad sites", 0, (t[0].b.base = 0, h1[2] = 2));
#undef BAD

    /* arguments that are no table at all */
    good(t, h1);
    expect("no context", c3r_set_phase_alleles(NULL, t, h1, 3, pool, 3), C3R_EINVAL, -1);
    expect("negative n", c3r_set_phase_alleles(ctx, t, h1, -1, pool, 3), C3R_EINVAL, -1);
    expect("no sites", c3r_set_phase_alleles(ctx, NULL, h1, 3, pool, 3), C3R_EINVAL, -1);
    expect("no h1", c3r_set_phase_alleles(ctx, t, NULL, 3, pool, 3), C3R_EINVAL, -1);
    expect("pool bases without a pool", c3r_set_phase_alleles(ctx, t, h1, 3, NULL, 3), C3R_EINVAL, -1);
    expect("negative pool", c3r_set_phase_alleles(ctx, t, h1, 3, pool, -1), C3R_EINVAL, -1);
    still_set("bad arguments", 1);

    /* one table at a time, and n = 0 through either setter clears it */
    c3r_phase_site_t p;
    memset(&p, 0, sizeof p);
    p.pos = 5; p.ps = 1; p.ref = 1; p.alt = 2;
    expect("the SNV setter after the allele setter", c3r_set_phase_sites(ctx, &p, 1), C3R_OK, -1);
    still_set("the SNV setter after the allele setter", 1);
    expect("n = 0 through the allele setter", c3r_set_phase_alleles(ctx, NULL, NULL, 0, NULL, 0), C3R_OK, -1);
    still_set("n = 0 through the allele setter", 0);
    expect("a table without insertions and without a pool", c3r_set_phase_alleles(ctx, t, h1, 1, NULL, 0), C3R_OK, -1);
    still_set("a table without insertions and without a pool", 1);
    expect("n = 0 through the SNV setter", c3r_set_phase_sites(ctx, NULL, 0), C3R_OK, -1);
    still_set("n = 0 through the SNV setter", 0);

    c3r_destroy(ctx);
    if (failures) { printf("phase_alleles_check: %d failure(s)\n", failures); return 1; }
    printf("phase_alleles_check: ok\n");
    return 0;
}
