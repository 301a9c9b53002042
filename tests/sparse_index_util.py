"""Building a sparse index (`kma index -Sparse`: index.c:451-474 / 576-613, makeindex.c:46-48 / 167-291, updateindex.c:79-199,
qualcheck.c:31-79, hashmap.c:120-187) restated in plain Python on strings, for the tests of kmahip_index_build_sparse, and the fixture
cases of tests/golden/sparse_index/ (made by tests/golden/make_golden_sparse_index.py). test_sparse_index_oracle.py pins the
restatement to the reference's own files. No test lives here.

The rule. A window is prefix_len + k consecutive bases of a trimmed template, or of its reverse complement, that hold no N and begin
with the prefix; its k-mer is its last k bases (no prefix: every N-free k-mer of either strand). slen = windows of the template over
both strands, ulen = its distinct window k-mers. A template stays iff MinLen < length, its windows reach MinKlen (no prefix:
(length - k + 1) * 2 stands for them) and slen > 0; one that goes has no id, no name and no .seq.b words."""
import gzip
import lzma
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_index")
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
INDEX = os.path.join(ROOT, "examples", "kmahip_index")
INPUTS = ("db1.fsa.gz", "db2.fsa.gz")

# case -> (k given with -k or None, the argument of -Sparse, -ML or 0)
CASES = {
    "k16_TG": (16, "TG", 0),
    "k16_none": (16, "-", 0),
    "k12_ATG": (12, "ATG", 0),
    "nok_TG": (None, "TG", 0),
    "k16_TG_ML60": (16, "TG", 60),
}
# the sparse indexes that the fixtures of sparse mapping already hold: name -> (folder under tests/golden/sparse, index name, FASTA)
OLD = {
    "se_TG": ("se", "TG", os.path.join(ROOT, "tests", "golden", "se", "db.fsa.gz"), "TG"),
    "se_none": ("se", "none", os.path.join(ROOT, "tests", "golden", "se", "db.fsa.gz"), "-"),
    "se_ATG": ("se", "ATG", os.path.join(ROOT, "tests", "golden", "se", "db.fsa.gz"), "ATG"),
    "e_TG": ("e", "TG", os.path.join(ROOT, "tests", "golden", "sparse", "e", "db.fsa.gz"), "TG"),
}

_LETTERS = {c: "ACGTN"[v] for v, cs in ((0, "AaRrMmDd"), (1, "CcYyBb"), (2, "GgSsKkVv"), (3, "TtWwHhUu"), (4, "NnXx")) for c in cs}
_COMP = str.maketrans("ACGTN", "TGCAN")
_VAL = {c: i for i, c in enumerate("ACGT")}


def kma_args(case):
    k, sp, ml = CASES[case]
    return (["-k", str(k)] if k else []) + ["-Sparse", sp] + (["-ML", str(ml)] if ml else [])


def read_fasta(path):
    """-> [(name, sequence over ACGTN with the ends trimmed of N, N's cut off the front)]: the letter table folds IUPAC codes and
    case, any other byte is passed over, the header loses its trailing blanks"""
    raw = (gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")).read().decode("latin-1")
    out = []
    for rec in raw.split(">")[1:]:
        head, _, body = rec.partition("\n")
        seq = "".join(_LETTERS.get(c, "") for c in body)
        lead = len(seq) - len(seq.lstrip("N"))
        out.append((head.rstrip(), seq.strip("N"), lead))
    return out


def encode(kmer):
    v = 0
    for c in kmer:
        v = (v << 2) | _VAL[c]
    return v


def windows(seq, k, prefix):
    """the window k-mers (strings) of one template, forward strand then reverse, repeats and all; prefix "" = none"""
    out = []
    w = len(prefix) + k
    for s in (seq, seq.translate(_COMP)[::-1]):
        for j in range(len(s) - w + 1):
            piece = s[j:j + w]
            if "N" not in piece and piece.startswith(prefix):
                out.append(piece[len(prefix):])
    return out


def gates(k, kmerindex, prefix_len, min_len):
    """-> (MinLen, MinKlen), index.c:599-606"""
    if min_len > k + prefix_len + 1:
        klen = 2 * (min_len - k - prefix_len + 1)
        for _ in range(prefix_len):
            klen //= 4
        return min_len, klen
    return max(k, kmerindex), 1


class Built:
    """what the rule makes of FASTA files: DB_size, names / lengths / slengths / ulengths (slot 0 as the files hold it), lists
    (k-mer -> ascending ids), skipped (names in file order), prefix_len and prefix as the .comp.b header holds them"""

    def __init__(self, paths, sparse, k=None, min_len=0):
        self.k = k or 16
        self.kmerindex = k or 16
        text = "" if sparse == "-" else "".join(_LETTERS[c] for c in sparse)
        assert sparse == "-" or (text and "N" not in text)
        self.prefix_len, self.prefix = len(text), (encode(text) if text else 1)
        MinLen, MinKlen = gates(self.k, self.kmerindex, len(text), min_len)
        self.names, self.lengths, self.slengths, self.ulengths = [None], [self.kmerindex], [0], [0]
        self.lists, self.skipped, self.seqs = {}, [], [None]
        for path in ([paths] if isinstance(paths, (str, bytes, os.PathLike)) else paths):
            for name, seq, lead in read_fasta(path):
                ws = windows(seq, self.k, text) if len(seq) >= self.k else []
                have = len(ws) if text else (len(seq) - self.k + 1) * 2
                if not (MinLen < len(seq) and have >= MinKlen and ws):
                    self.skipped.append(name)
                    continue
                tid = len(self.names)
                uniq = set(ws)
                for km in uniq:
                    self.lists.setdefault(encode(km), []).append(tid)
                self.names.append(name + (" B%d" % lead if lead else ""))
                self.lengths.append(len(seq)); self.slengths.append(len(ws)); self.ulengths.append(len(uniq))
                self.seqs.append(seq)
        self.DB_size = len(self.names)

    def length_b(self):
        return struct.pack("<I", self.DB_size) + b"".join(np.array(a, np.uint32).tobytes() for a in (self.lengths, self.slengths, self.ulengths))

    def name_file(self):
        return "".join(n + "\n" for n in self.names[1:]).encode()

    def seq_words(self):
        """per template the words of .seq.b that carry bases (N as A), 32 bases a word from the top"""
        out = []
        for s in self.seqs[1:]:
            ws = []
            for a in range(0, len(s), 32):
                piece = s[a:a + 32].replace("N", "A")
                ws.append(encode(piece) << (2 * (32 - len(piece))))
            out.append(ws)
        return out


class Files:
    """an index on disk as the comparisons need it: the .comp.b header, key -> ascending ids, and the raw .length.b / .name"""

    def __init__(self, prefix):
        b = open(prefix + ".comp.b", "rb").read()
        self.DB_size, self.mlen, self.prefix_len = struct.unpack_from("<3I", b, 0)
        self.prefix, self.size, self.n, self.v_index, _ = struct.unpack_from("<5Q", b, 12)
        o = 52 + 4 * self.size
        vdt = np.uint16 if self.DB_size < 65535 else np.uint32
        assert self.size != 1 << (2 * self.mlen), "direct-addressed form: not what these fixtures hold"
        values = np.frombuffer(b, vdt, self.v_index, o).astype(np.int64).tolist(); o += self.v_index * np.dtype(vdt).itemsize
        keys = np.frombuffer(b, np.uint32, self.n + 1, o)[:self.n].tolist(); o += 4 * (self.n + 1)
        vidx = np.frombuffer(b, np.uint32, self.n, o).tolist(); o += 4 * self.n
        self.k, self.flag = struct.unpack_from("<2I", b, o)
        self.lists = {key: values[vi + 1:vi + 1 + values[vi]] for key, vi in zip(keys, vidx)}
        self.length_b = open(prefix + ".length.b", "rb").read()
        self.name_file = open(prefix + ".name", "rb").read()
        raw = np.frombuffer(self.length_b, np.uint32)
        D = self.DB_size
        assert int(raw[0]) == D and len(raw) == 1 + 3 * D
        self.lengths, self.slengths, self.ulengths = (raw[1 + i * D:1 + (i + 1) * D].tolist() for i in range(3))


def unpack(src_dir, name, dst, with_seq=True):
    """a stored index (name.comp.b.xz, name.length.b, name.name[, name.seq.b]) into folder dst -> its prefix"""
    prefix = os.path.join(str(dst), "ref_" + name)
    with lzma.open(os.path.join(src_dir, name + ".comp.b.xz"), "rb") as f, open(prefix + ".comp.b", "wb") as g:
        g.write(f.read())
    for ext in (".length.b", ".name") + ((".seq.b",) if with_seq else ()):
        with open(os.path.join(src_dir, name + ext), "rb") as f, open(prefix + ext, "wb") as g:
            g.write(f.read())
    return prefix


def inputs():
    return [os.path.join(GOLDEN, f) for f in INPUTS]


def skipped(case):
    return open(os.path.join(GOLDEN, case + ".skipped.txt")).read().split("\n")[:-1]


def seq_words_equal(got_path, ref_path, lengths):
    """.seq.b word for word over the words that carry bases: when a length is a multiple of 32 the reference's last word is whatever
    its buffer held before (updateindex.c:187 writes one word more than compDNAref filled)"""
    wa, wb = np.fromfile(got_path, np.uint64), np.fromfile(ref_path, np.uint64)
    lens = np.asarray(lengths, np.int64)
    assert len(wa) == len(wb) == int(((lens >> 5) + 1).sum()), (len(wa), len(wb))
    o = 0
    for L in lens.tolist():
        w = (L + 31) >> 5
        assert np.array_equal(wa[o:o + w], wb[o:o + w]), o
        o += (L >> 5) + 1
