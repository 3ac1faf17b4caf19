"""What bam.write_bam writes for a fixed ReadSet WITHOUT qualities, as a hash: tests/test_hap_min_bq_ref.py holds it against
tests/golden/hap_min_bq_parent_bytes.json, which was recorded by running this file with the parent commit's package.  It imports nothing of
tests/ and takes the package from sys.path, so that it can be run against another tree:

    PYTHONPATH=<tree> python tests/support/bam_bytes.py <scratch directory>

Hashed: the inflated payload of the file, block by block with every block's length (the deflate stream itself depends on the zlib at hand)."""
import hashlib
import json
import os
import random
import sys


def records():
    """130 reads over two contigs' worth of positions: lengths 1 .. 40 (odd and even), indels, clips, a ref-skip, HP tags."""
    rnd = random.Random(7)
    out = []
    for k in range(130):
        L = 1 + k % 40
        seq = "".join(rnd.choice("ACGTN") for _ in range(L))
        if L >= 12 and k % 3 == 0:
            cigar = "2S%dM1I3M2D%dM50N2M" % (3, L - 11)
        else:
            cigar = "%dM" % L
        out.append(dict(pos=10 * k + rnd.randrange(5), cigar=cigar, seq=seq, flag=16 * (k % 2), mapq=rnd.randrange(61), hp=k % 3))
    return out


def bam_hash(out_dir):
    from clair3_rna_amd import bam
    from clair3_rna_amd.reads import ReadSet
    rs = ReadSet.from_records(records())
    fn = os.path.join(out_dir, "no_quals.bam")
    bam.write_bam(fn, [("chr1", 5000), ("chr2", 5000)], {"chr1": rs, "chr2": rs})
    h = hashlib.sha256()
    for block in bam._bgzf_blocks(fn):
        h.update(len(block).to_bytes(4, "little") + block)
    os.remove(fn)
    return h.hexdigest()


if __name__ == "__main__":
    print(json.dumps({"write_bam/no_quals.bam": bam_hash(sys.argv[1])}, indent=1))
