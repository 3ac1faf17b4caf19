#!/usr/bin/env python3
"""What the per-haplotype allele counts cost (c3r_hap_counts / k_hap_counts, c3r_hap_allele_counts / k_hap_allele_counts) beside the kernels
that read the same records once, and what the extra store of the read's phase set costs k_haplotag.

    python tools/hapcount_time.py [--commit ID] [--out profiles/hap_counts.txt] [--rounds 10] [--only phased,stress]
                                  [--parent_root DIR [--ab_loads phased,stress] [--ab haplotag|counts]]

The loads are tools/phase_time.py's (`phased`: BASELINE.json configs[3], MAS-Seq chr20 ~30x; `stress`: configs[4], loci at ~500x; `deep`:
loci at ~20,000x, not in the default list), and so are the candidates: pass 1's own heterozygous SNVs through synth.random_weights.  The
phase table is what the chain (Engine.phase_sites) makes of them; the query sites are ALL candidates, each with the set of the nearest
table site (hap_vcf.nearest_sets) — what hap_vcf asks.

Per load, written to --out (appended):
    k_hap_counts and k_hap_allele_counts (the same SNV-only query) beside k_phase_links, k_haplotag and k_prep_count
                                                                       ms per launch (profiling on; mean over the rounds), same reads, same run
    Engine.hap_counts wall time beside Engine.load_reads              ms, median and min .. max (profiling off)
--parent_root DIR: a built tree of the parent commit.  k_haplotag is then timed in child processes that alternate between this tree and
that one (three of each), every child on the same reads under the same table (saved by this process): the extra store against the
run-to-run spread.
--ab counts (with --parent_root): instead, k_hap_counts of that tree against k_hap_counts and k_hap_allele_counts of this one on the same
SNV-only query, and k_hap_allele_counts (that tree's too, where it has the kernel) on an INDEL query of the same size (indel_query: the insertions and deletions that most reads show
behind an M op, each as a 0/1 site), in alternating child processes on the reads, table and queries that this process saved.  This
process skips its own kernel and wall-time sections then: the children are the measurement."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def haplotag_child(root, name, table_fn, rounds):
    """One process: k_haplotag ms per launch over `rounds` loads of `name` under the saved table, with the package of `root`."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import phase_time                                        # (puts this tree first on the path: `root` goes before it afterwards)
    sys.path.insert(0, os.path.abspath(root))
    from clair3_rna_amd import capi, synth
    assert os.path.abspath(capi.__file__).startswith(os.path.abspath(root) + os.sep), capi.__file__
    _title, gen, L = phase_time.LOADS[name]
    gen = dict(gen)
    L = L or synth.CHR20_LEN
    _ref, rs, _info = synth.generate_contig(contig_len=L, seed=synth.SEED + gen.pop("seed_off"), **gen)
    rs = capi.pinned_readset(rs)
    eng = capi.Engine(0)
    eng.set_params()
    eng.set_phase_sites(np.load(table_fn))
    eng.load_reads(rs)                                       # (first use: buffers)
    eng.set_profiling(True)
    ms = []
    for _ in range(rounds):
        eng.reset_kernel_stats()
        eng.load_reads(rs)
        eng.synchronize()
        k = eng.kernel_stats()["k_haplotag"]
        ms.append(k["total_ms"] / k["launches"])
    eng.close()
    print("HAPLOTAG_MS %s" % " ".join("%.4f" % v for v in ms), flush=True)


def indel_query(rs, n, table):
    """(HAP_SITE_DTYPE array, packed pool): up to n sites on the positions where most reads show an insertion (1-6 bases) or a deletion
    (1-6) directly behind an M / = / X op, each a 0/1 site whose ALT is what the first such read shows, with the nearest table site's set."""
    from clair3_rna_amd import capi, hap_vcf
    cig = np.asarray(rs.cigar)
    op, ln = (cig & 15).astype(np.int64), (cig >> 4).astype(np.int64)
    owner = np.repeat(np.arange(len(rs.reads)), rs.reads["n_cigar"].astype(np.int64))
    first = rs.reads["cigar_off"].astype(np.int64)[owner]
    is_m = (op == 0) | (op == 7) | (op == 8)
    cr = np.cumsum(np.where(is_m | (op == 2) | (op == 3), ln, 0))
    cq = np.cumsum(np.where(is_m | (op == 1) | (op == 4), ln, 0))
    idx = np.arange(len(cig))
    prev_m = np.zeros(len(cig), bool)
    prev_m[1:] = is_m[:-1] & (owner[1:] == owner[:-1])
    nxt_d = np.zeros(len(cig), bool)
    nxt_d[:-1] = (op[1:] == 2) & (owner[1:] == owner[:-1])
    hit = np.flatnonzero(prev_m & (ln >= 1) & (ln <= 6) & (((op == 1) & ~nxt_d) | (op == 2)))
    base_r = np.where(first > 0, cr[np.maximum(first - 1, 0)], 0)
    base_q = np.where(first > 0, cq[np.maximum(first - 1, 0)], 0)
    anchor = rs.reads["pos"].astype(np.int64)[owner[hit]] + (cr[hit] - np.where((op[hit] == 2), ln[hit], 0) - base_r[hit])      # 1-based last base of the M op
    qoff = cq[hit] - np.where(op[hit] == 1, ln[hit], 0) - base_q[hit]                                                          # query offset of the inserted bases
    pos, where, count = np.unique(anchor, return_index=True, return_counts=True)
    take = np.sort(np.argsort(-count, kind="stable")[:n])
    sites = np.zeros(len(take), dtype=capi.HAP_SITE_DTYPE)
    pool = []
    for k, t in enumerate(take):
        h = hit[where[t]]
        r = rs.reads[owner[h]]
        sites[k]["pos"], sites[k]["event_matters"], sites[k]["a_base"], sites[k]["b_base"] = pos[t], 1, 1, 1      # (the base does not matter: A)
        sites[k]["b_kind"], sites[k]["b_len"] = (capi.HAP_EV_INS if op[h] == 1 else capi.HAP_EV_DEL), ln[h]
        if op[h] == 1:
            codes = [(int(rs.seq[int(r["seq_off"]) + (q >> 1)]) >> (0 if q & 1 else 4)) & 15 for q in range(int(qoff[where[t]]), int(qoff[where[t]] + ln[h]))]
            if any(c not in (1, 2, 4, 8) for c in codes) or int(qoff[where[t]] + ln[h]) > int(r["l_seq"]):
                sites[k]["b_kind"], sites[k]["b_len"] = capi.HAP_EV_DEL, 1
            else:
                sites[k]["b_ins_off"] = len(pool)
                pool += codes
    return hap_vcf.nearest_sets(sites, table), capi.pack_nibbles(pool)


def counts_child(root, scratch, name, rounds):
    """One process: ms per launch of k_hap_counts — and, where the package of `root` has it, of k_hap_allele_counts on the same SNV-only query
    and on the indel query — over `rounds` calls on the saved reads, table and queries of `name`."""
    sys.path.insert(0, os.path.abspath(root))
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    assert os.path.abspath(capi.__file__).startswith(os.path.abspath(root) + os.sep), capi.__file__
    z = np.load(os.path.join(scratch, "hapcount_%s.npz" % name))
    rs = ReadSet.__new__(ReadSet)
    rs.reads, rs.cigar, rs.seq = z["reads"], z["cigar"], z["seq"]
    rs = capi.pinned_readset(rs)
    eng = capi.Engine(0)
    eng.set_params()
    eng.set_phase_sites(z["table"])
    eng.load_reads(rs)
    query = z["query"]
    calls = [("k_hap_counts", "HAP_COUNTS_MS", lambda: eng.hap_counts(query))]
    if hasattr(eng, "hap_allele_counts"):
        as_alleles = capi.hap_sites_from_snvs(query)
        assert np.array_equal(eng.hap_allele_counts(as_alleles), eng.hap_counts(query))
        calls.append(("k_hap_allele_counts", "HAP_ALLELE_SNV_MS", lambda: eng.hap_allele_counts(as_alleles)))
        calls.append(("k_hap_allele_counts", "HAP_ALLELE_INDEL_MS", lambda: eng.hap_allele_counts(z["indel_query"], z["indel_pool"])))
    for _, _, call in calls:
        call()                                               # (first use: buffers)
    eng.set_profiling(True)
    for kernel, label, call in calls:
        ms = []
        for _ in range(rounds):
            eng.reset_kernel_stats()
            call()
            k = eng.kernel_stats()[kernel]
            ms.append(k["total_ms"] / k["launches"])
        print("%s %s" % (label, " ".join("%.4f" % v for v in ms)), flush=True)
    eng.close()


def counts_ab(name, rounds, parent_root, scratch, rs, table, query):
    """The lines of the A/B of the two kernels on one load: three children of this tree and three of the parent's, taking turns."""
    indel, pool = indel_query(rs, len(query), table)
    os.makedirs(scratch, exist_ok=True)
    np.savez(os.path.join(scratch, "hapcount_%s.npz" % name), reads=np.asarray(rs.reads), cigar=np.asarray(rs.cigar), seq=np.asarray(rs.seq), table=table,
             query=query, indel_query=indel, indel_pool=pool)
    n_ins = int((indel["b_kind"] == 1).sum())
    lines = ["   A/B of the count kernels: SNV query of %d sites; indel query of %d sites (%d insertions, %d deletions)" % (len(query), len(indel), n_ins, len(indel) - n_ins)]
    runs = {}
    for k in range(6):                                       # this, parent, this, parent, ...: fresh processes, one at a time
        who = "this" if k % 2 == 0 else "parent"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--counts_child", ROOT if who == "this" else parent_root, "--only", name,
                            "--scratch", scratch, "--rounds", str(rounds)], stdout=subprocess.PIPE, text=True, timeout=300)
        got = [l.split() for l in r.stdout.split("\n") if l.startswith("HAP_")]
        if r.returncode != 0 or not got:
            lines.append("   A/B of the count kernels: the %s child ended with %d: stopped" % (who, r.returncode))
            break
        for g in got:
            runs.setdefault((who, g[0]), []).append(float(np.mean([float(v) for v in g[1:]])))
    for (who, label), title in ((("parent", "HAP_COUNTS_MS"), "parent commit  k_hap_counts                     "),
                                (("this", "HAP_COUNTS_MS"), "this commit    k_hap_counts                     "),
                                (("parent", "HAP_ALLELE_SNV_MS"), "parent commit  k_hap_allele_counts, SNV query   "),
                                (("parent", "HAP_ALLELE_INDEL_MS"), "parent commit  k_hap_allele_counts, indel query "),
                                (("this", "HAP_ALLELE_SNV_MS"), "this commit    k_hap_allele_counts, SNV query   "),
                                (("this", "HAP_ALLELE_INDEL_MS"), "this commit    k_hap_allele_counts, indel query ")):
        lines.append("   %s ms per launch, alternating processes (mean of %d calls each): %s" % (title, rounds, " ".join("%.4f" % v for v in runs.get((who, label), []))))
    return lines


def time_load(name, rounds, parent_root, scratch, ab="haplotag"):
    """The lines of one load; parent_root None: no A/B of k_haplotag."""
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    from clair3_rna_amd import capi, hap_vcf, synth
    title, gen, L = phase_time.LOADS[name]
    gen = dict(gen)
    L = L or synth.CHR20_LEN
    ref, rs, _info = synth.generate_contig(contig_len=L, seed=synth.SEED + gen.pop("seed_off"), **gen)
    rs = capi.pinned_readset(rs)
    eng = capi.Engine(0)
    eng.set_params()
    eng.load_reads(rs)
    sites, what = phase_time.pass1_candidates(eng, ref, L)
    lines = ["-- %s (%s): %d reads, %d CIGAR ops; %s" % (name, title, len(rs.reads), len(rs.cigar), what)]
    out, st = eng.phase_sites(sites) if len(sites) else (sites, dict(n_phased=0))
    if not st["n_phased"]:
        eng.close()
        return lines + ["   no phased sites: nothing to time"]
    table = np.ascontiguousarray(out[out["ps"] >= 0])
    query = hap_vcf.nearest_sets(sites, table)
    eng.set_phase_sites(table)
    counts = eng.hap_counts(query)
    _, ast = capi.hap_assign(query, counts)
    lines.append("   table: %d sites in %d sets; %d query sites; observations by row (none, hp1, hp2): %s; hap_assign: %s"
                 % (len(table), len(set(table["ps"].tolist())), len(query), counts.sum(axis=(0, 2)).tolist(), ast))
    if parent_root and ab == "counts":
        eng.close()
        return lines + counts_ab(name, rounds, parent_root, scratch, rs, table, query)
    as_alleles = capi.hap_sites_from_snvs(query)
    assert np.array_equal(eng.hap_allele_counts(as_alleles), counts)
    eng.set_profiling(True)
    kern = {}
    for _ in range(rounds):
        eng.reset_kernel_stats()
        eng.load_reads(rs)                                   # under the table: k_prep_count, k_haplotag, k_prep_write
        eng.phase_links(sites)
        eng.hap_counts(query)
        eng.hap_allele_counts(as_alleles)                    # the same SNV-only query through the general kernel
        for k, v in eng.kernel_stats().items():
            kern.setdefault(k, []).append(v["total_ms"] / max(1, v["launches"]))
    eng.set_profiling(False)
    lines.append("   kernels, ms per launch (profiling on, mean of %d): %s" % (
        rounds, "  ".join("%s %.4f" % (k, float(np.mean(kern[k]))) for k in ("k_hap_counts", "k_hap_allele_counts", "k_phase_links", "k_haplotag", "k_prep_count", "k_prep_write") if k in kern)))
    w_load, w_count = [], []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        w_load.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        eng.hap_counts(query)
        w_count.append(1e3 * (time.perf_counter() - t0))
    eng.close()
    lines.append("   Engine.load_reads  wall ms (profiling off, table set): %s" % phase_time.spread(w_load))
    lines.append("   Engine.hap_counts  wall ms (profiling off): %s" % phase_time.spread(w_count))
    if parent_root:
        os.makedirs(scratch, exist_ok=True)
        table_fn = os.path.join(scratch, "hapcount_table_%s.npy" % name)
        np.save(table_fn, table)
        runs = {"this": [], "parent": []}
        for k in range(6):                                   # this, parent, this, parent, ...: fresh processes, one at a time
            who = "this" if k % 2 == 0 else "parent"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--haplotag_child", ROOT if who == "this" else parent_root, "--only", name,
                                "--table", table_fn, "--rounds", str(rounds)], stdout=subprocess.PIPE, text=True, timeout=300)
            got = [l for l in r.stdout.split("\n") if l.startswith("HAPLOTAG_MS ")]
            if r.returncode != 0 or not got:
                lines.append("   k_haplotag A/B: the %s child ended with %d: stopped" % (who, r.returncode))
                break
            runs[who].append(float(np.mean([float(v) for v in got[0].split()[1:]])))
        lines.append("   k_haplotag ms per launch, alternating processes (mean of %d loads each): this commit %s | parent commit %s" % (
            rounds, " ".join("%.4f" % v for v in runs["this"]), " ".join("%.4f" % v for v in runs["parent"])))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_counts.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", default="phased,stress")
    ap.add_argument("--parent_root", default=None, help="a built tree of the parent commit: k_haplotag there against here")
    ap.add_argument("--ab_loads", default="phased,stress", help="the loads on which k_haplotag is timed against --parent_root")
    ap.add_argument("--scratch", default=None, help="where the table of the A/B children is kept (default: a fresh temporary directory)")
    ap.add_argument("--ab", default="haplotag", choices=("haplotag", "counts"), help="what is timed against --parent_root")
    ap.add_argument("--haplotag_child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--counts_child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--table", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.haplotag_child:
        return haplotag_child(a.haplotag_child, a.only, a.table, a.rounds)
    if a.counts_child:
        return counts_child(a.counts_child, a.scratch, a.only, a.rounds)
    if a.scratch is None:
        import tempfile
        a.scratch = tempfile.mkdtemp(prefix="hapcount_time_")
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    emit(["== hapcount_time: commit %s, %d rounds" % (a.commit or phase_time.commit_id(), a.rounds)])
    for name in a.only.split(","):
        emit(time_load(name, a.rounds, a.parent_root if name in a.ab_loads.split(",") else None, a.scratch, a.ab))


if __name__ == "__main__":
    main()
