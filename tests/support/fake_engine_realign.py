"""A logging stand-in for capi.Engine, for the driver tests of --hap_realign that need no GPU (tests/test_realign_ref.py): it records the
order of the calls a driver makes and answers with empty results of the right shapes."""
import numpy as np


class Engine(object):
    log = []

    def __init__(self, device=0):
        pass

    def close(self):
        pass

    def set_params(self, **kw):
        pass

    def set_reference(self, start, seq):
        Engine.log.append(("reference", start, len(seq)))

    def set_hap_realign(self, overhang):
        Engine.log.append(("realign", overhang))

    def set_hap_left_align(self, on):
        Engine.log.append(("left_align", on))

    def set_hap_min_bq(self, q):
        Engine.log.append(("min_bq", q))

    def load_reads(self, rs):
        Engine.log.append(("reads", len(rs)))

    def set_phase_sites(self, sites):
        Engine.log.append(("snv_table", 0 if sites is None else len(sites)))

    def set_phase_alleles(self, sites, h1, pool=None, pool_bases=None):
        Engine.log.append(("allele_table", 0 if sites is None else len(sites), [int(b) for b in sites["base_matters"]], [int(h) for h in h1]))

    def phase_sites(self, sites, min_reads, min_agree_pct, merge_levels):
        Engine.log.append(("phase_snv", [int(p) for p in sites["pos"]]))
        out = sites.copy()
        out["ps"], out["h1"] = 3, 0
        return out, dict(n_sites=len(sites), n_phased=len(sites), n_blocks=1, max_block=len(sites))

    def phase_allele_sites(self, sites, pool, min_reads, min_agree_pct, merge_levels):
        Engine.log.append(("phase_alleles", [int(p) for p in sites["pos"]], [(int(s["a_base"]), int(s["b_base"]), int(s["base_matters"]), int(s["event_matters"])) for s in sites]))
        n = len(sites)
        return np.full(n, 3, np.int32), np.zeros(n, np.uint8), dict(n_sites=n, n_phased=n, n_blocks=1, max_block=n)

    def haplotags(self):
        return np.zeros(1, np.uint8), {}

    def read_phase_sets(self):
        return np.full(1, -1, np.int32)
