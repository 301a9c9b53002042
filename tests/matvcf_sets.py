"""Input set V of the count-matrix / VCF tests (tests/golden/matvcf_v holds the reference's two files for it), shared by the GPU tests
of test_matvcf_gpu.py and the CPU test that pins the oracle's columns on the recorded matrix. No test lives here.

V, by hand: three templates of 300 bases (default_rng(99)), 20 reads over positions 20 .. 171 of template 1; every read substitutes
position 50 and deletes position 110, reads 0-7 substitute position 140, reads 0-13 insert two bases behind position 80, reads 14-16
insert one base behind position 125; cut to 150 bases."""
import numpy as np


def v_templates():
    rng = np.random.default_rng(99)
    return ["hand%d" % i for i in range(3)], [rng.integers(0, 4, 300, dtype=np.uint8) for _ in range(3)]


def v_reads(seqs):
    s = seqs[1]
    reads = []
    for i in range(20):
        r = []
        for pos in range(20, 172):
            if pos == 110:
                continue
            b = int(s[pos])
            if pos == 50:
                b = (b + 1) & 3
            if pos == 140 and i < 8:
                b = (b + 2) & 3
            r.append(b)
            if pos == 80 and i < 14:
                r += [(int(s[81]) + 1) & 3, (int(s[81]) + 2) & 3]
            if pos == 125 and 14 <= i <= 16:
                r.append((int(s[126]) + 1) & 3)
        reads.append(np.array(r[:150], np.uint8))
    return reads
