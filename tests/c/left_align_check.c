/* left_align_check.c — c3r_hap_left_align_sites through the C ABI alone: the hand-derived tables of tests/test_leftalign_ref.py (a
 * homopolymer deletion, a rotated dinucleotide insertion, a 1/2 site of two deletions, an SNV beside a deletion in a tract, a collision,
 * a tract at the slice's edge, an N inside a tract), the refusals and the overflow.  Host code only: no context, no device.  Built as
 * plain C against include/c3r.h and libc3r.so:
 *   cc -std=c11 -Wall -Iinclude tests/c/left_align_check.c -Lclair3_rna_amd -lc3r -Wl,-rpath,<dir of libc3r.so> -o left_align_check
 * Prints "left_align_check: ok" and exits 0, or says what differed and exits 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3r.h"

static int failures = 0;

static void check(const char *name, int ok) {
    if (!ok) { printf("left_align_check: %s FAILED\n", name); failures += 1; }
}

static c3r_hap_site_t site(int32_t pos, int32_t ps) {
    c3r_hap_site_t s;
    memset(&s, 0, sizeof s);
    s.pos = pos; s.ps = ps;
    return s;
}
static c3r_hap_allele_t allele(uint8_t base, uint8_t kind, uint16_t len, uint32_t off) {
    c3r_hap_allele_t a;
    a.base = base; a.kind = kind; a.len = len; a.ins_off = off;
    return a;
}
/* REF and one indel ALT behind the same anchor base */
static c3r_hap_site_t indel(int32_t pos, uint8_t base, uint8_t kind, uint16_t len, uint32_t off) {
    c3r_hap_site_t s = site(pos, 7);
    s.event_matters = 1;
    s.a = allele(base, C3R_HAP_EV_NONE, 0, 0);
    s.b = allele(base, kind, len, off);
    return s;
}
static uint8_t nib(const uint8_t *p, int64_t q) { return (q & 1) ? (uint8_t)(p[q >> 1] & 15) : (uint8_t)(p[q >> 1] >> 4); }

#define A 1
#define C 2
#define G 4
#define T 8

int main(void) {
    /*                      0-based: 01234567 */
    const char *homo = "GCAAAATC";  /* AAAA on 2 .. 5 behind a C  */
    const char *dinuc = "tgacacacgt"; /* (AC)3 on 2 .. 7 behind a G, lower case on purpose */
    const char *with_n = "GCAANAATC";
    c3r_hap_site_t in[4], out[4];
    uint8_t pool[4], opool[4];
    int64_t src[4], n_out = -1, nb = -1;
    c3r_left_align_stats_t st;
    int rc;

    /* AA > A on 5 (anchor 0-based 4): three shifts, the C on 1 */
    in[0] = indel(5, A, C3R_HAP_EV_DEL, 1, 0);
    rc = c3r_hap_left_align_sites(in, 1, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, &n_out, &st);
    check("homopolymer_del", rc == C3R_OK && n_out == 1 && nb == 0 && src[0] == 0 && out[0].pos == 2 && out[0].ps == 7 && out[0].a.base == C && out[0].b.base == C &&
                                 out[0].b.kind == C3R_HAP_EV_DEL && out[0].b.len == 1 && out[0].event_matters == 1 && out[0].base_matters == 0 && st.n_in == 1 &&
                                 st.n_out == 1 && st.n_moved == 1 && st.n_not_left_alignable == 0 && st.n_same_pos_after_left_align == 0);

    /* A > ACA on 5 (anchor 4, INS CA; the pool holds a leading T so that the offset is odd): three shifts, INS AC behind the G on 1 */
    pool[0] = (T << 4) | C; pool[1] = (A << 4);
    in[0] = indel(5, A, C3R_HAP_EV_INS, 2, 1);
    memset(opool, 0xff, sizeof opool);
    rc = c3r_hap_left_align_sites(in, 1, pool, 3, 1, dinuc, 10, out, opool, 2, &nb, src, &n_out, &st);
    check("dinucleotide_ins_rotated", rc == C3R_OK && n_out == 1 && nb == 2 && out[0].pos == 2 && out[0].a.base == G && out[0].b.base == G && out[0].b.kind == C3R_HAP_EV_INS &&
                                          out[0].b.len == 2 && out[0].b.ins_off == 0 && nib(opool, 0) == A && nib(opool, 1) == C && st.n_moved == 1);
    rc = c3r_hap_left_align_sites(in, 1, pool, 3, 1, dinuc, 10, out, opool, 1, &nb, src, &n_out, &st);
    check("pool_overflow", rc == C3R_EOVERFLOW);

    /* AAA > AA,A on 4: DEL 1 and DEL 2 both shift twice */
    in[0] = site(4, 0);
    in[0].event_matters = 1;
    in[0].a = allele(A, C3R_HAP_EV_DEL, 1, 0);
    in[0].b = allele(A, C3R_HAP_EV_DEL, 2, 0);
    rc = c3r_hap_left_align_sites(in, 1, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, &n_out, &st);
    check("two_deletions", rc == C3R_OK && n_out == 1 && out[0].pos == 2 && out[0].a.base == C && out[0].a.len == 1 && out[0].b.len == 2 && st.n_moved == 1);

    /* AA > TA,A on 4: the SNV pins the anchor, the deletion would shift twice */
    in[0] = site(4, 0);
    in[0].base_matters = 1; in[0].event_matters = 1;
    in[0].a = allele(T, C3R_HAP_EV_NONE, 0, 0);
    in[0].b = allele(A, C3R_HAP_EV_DEL, 1, 0);
    rc = c3r_hap_left_align_sites(in, 1, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, &n_out, &st);
    check("snv_and_indel_in_a_tract", rc == C3R_OK && n_out == 0 && st.n_not_left_alignable == 1 && st.n_moved == 0 && st.n_out == 0);

    /* the same deleted A on 5 and on 4, and an SNV on 7, handed in unsorted: the first in input order stays, the table comes back sorted */
    in[0] = site(7, 1);
    in[0].base_matters = 1;
    in[0].a = allele(T, C3R_HAP_EV_NONE, 0, 0);
    in[0].b = allele(G, C3R_HAP_EV_NONE, 0, 0);
    in[1] = indel(5, A, C3R_HAP_EV_DEL, 1, 0);
    in[2] = indel(4, A, C3R_HAP_EV_DEL, 1, 0);
    rc = c3r_hap_left_align_sites(in, 3, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, &n_out, &st);
    check("collision", rc == C3R_OK && n_out == 2 && out[0].pos == 2 && src[0] == 1 && out[1].pos == 7 && src[1] == 0 && out[1].ps == 1 && out[1].b.base == G &&
                           st.n_moved == 2 && st.n_same_pos_after_left_align == 1 && st.n_out == 2);

    /* the slice starts on 0-based 2 (ref_start 3): two shifts, the anchor is the A on 2 */
    in[0] = indel(5, A, C3R_HAP_EV_DEL, 1, 0);
    rc = c3r_hap_left_align_sites(in, 1, NULL, 0, 3, homo + 2, 6, out, NULL, 0, &nb, src, &n_out, &st);
    check("tract_at_slice_edge", rc == C3R_OK && n_out == 1 && out[0].pos == 3 && out[0].a.base == A);
    /* no slice at all: nothing moves */
    rc = c3r_hap_left_align_sites(in, 1, NULL, 0, 1, NULL, 0, out, NULL, 0, &nb, src, &n_out, &st);
    check("empty_slice", rc == C3R_OK && n_out == 1 && out[0].pos == 5 && st.n_moved == 0);

    /* A > AA on 7 (anchor 6): one shift, then the anchor would move onto the N */
    pool[0] = (A << 4);
    in[0] = indel(7, A, C3R_HAP_EV_INS, 1, 0);
    rc = c3r_hap_left_align_sites(in, 1, pool, 1, 1, with_n, 9, out, opool, 1, &nb, src, &n_out, &st);
    check("n_inside_a_tract", rc == C3R_OK && n_out == 1 && out[0].pos == 6 && out[0].a.base == A && nb == 1 && nib(opool, 0) == A);

    /* refusals */
    in[0] = indel(5, A, C3R_HAP_EV_DEL, 1, 0);
    in[0].pos = 0;
    check("refuses_pos_0", c3r_hap_left_align_sites(in, 1, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, &n_out, &st) == C3R_EINVAL);
    in[0] = indel(5, A, 3, 1, 0);
    check("refuses_unknown_kind", c3r_hap_left_align_sites(in, 1, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, &n_out, &st) == C3R_EINVAL);
    in[0] = indel(5, A, C3R_HAP_EV_DEL, 0, 0);
    check("refuses_length_0", c3r_hap_left_align_sites(in, 1, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, &n_out, &st) == C3R_EINVAL);
    in[0] = indel(5, A, C3R_HAP_EV_INS, 2, 2);
    check("refuses_insertion_past_pool", c3r_hap_left_align_sites(in, 1, pool, 3, 1, dinuc, 10, out, opool, 2, &nb, src, &n_out, &st) == C3R_EINVAL);
    check("refuses_ref_start_0", c3r_hap_left_align_sites(in, 0, NULL, 0, 0, homo, 8, out, NULL, 0, &nb, src, &n_out, &st) == C3R_EINVAL);
    check("refuses_no_count", c3r_hap_left_align_sites(in, 0, NULL, 0, 1, homo, 8, out, NULL, 0, &nb, src, NULL, &st) == C3R_EINVAL);
    /* n = 0, and the optional outputs left out */
    rc = c3r_hap_left_align_sites(NULL, 0, NULL, 0, 1, homo, 8, NULL, NULL, 0, NULL, NULL, &n_out, NULL);
    check("empty_table", rc == C3R_OK && n_out == 0);

    if (failures) return 1;
    printf("left_align_check: ok\n");
    return 0;
}
