"""Appending to an index (`kma index -t_db`: index.c:221-229, 529-557, 616-732; load_DBs and hashMapKMA_openChains, loadupdate.c)
restated in plain Python, for the tests of kmahip_index_append, and the fixture cases of tests/golden/index_append/ (made by
tests/golden/make_golden_index_append.py). test_index_append_oracle.py pins the restatement to the reference's own files. No test
lives here.

The rule. An append gives the index a fresh build of the old templates followed by the new ones gives. k and the sparse prefix are
the old index's. The k-mers of the old templates are those of the old .comp.b (`expand`): .seq.b stores an N as A and cannot give
them back. The new templates get the ids from the old DB_size on and are parsed as in a fresh build."""
import gzip
import lzma
import os
import struct

import numpy as np

import sparse_index_util as siu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "index_append")
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
INDEX = os.path.join(ROOT, "examples", "kmahip_index")
MAP = os.path.join(ROOT, "examples", "kmahip_map")

# the old indexes of the fixture, all built from a.fsa.gz: name -> arguments of `kma index`
OLD = {
    "A_k16": ["-k", "16"],
    "A_k12": ["-k", "12"],
    "A_TG": ["-k", "16", "-Sparse", "TG"],
    "A_none": ["-k", "16", "-Sparse", "-"],
    "A_k10": ["-k", "10"],          # 4^10 <= the reference's initial table: it writes the direct-address form
}
# case -> old: the index appended to; steps: the FASTA parts of each append in turn; line: what else stands on the command line (k and
# the prefix are the index's whatever it says); decon: with -deCon c.fsa.gz on the last step; inplace: no -o; want: the recorded result
CASES = {
    "k16": dict(old="A_k16", steps=[["b"]], line=[], want="k16"),
    "k12_with_k16_on_the_line": dict(old="A_k12", steps=[["b"]], line=["-k", "16"], want="k12"),
    "TG_with_the_option": dict(old="A_TG", steps=[["b"]], line=["-Sparse", "TG"], want="TG"),
    "TG_without_the_option": dict(old="A_TG", steps=[["b"]], line=[], want="TG"),
    "no_prefix": dict(old="A_none", steps=[["b"]], line=[], want="none"),
    "in_place": dict(old="A_k16", steps=[["b"]], line=[], inplace=True, want="k16"),
    "two_in_a_row": dict(old="A_k16", steps=[["b1"], ["b2"]], line=[], want="k16"),
    "two_files_at_once": dict(old="A_k16", steps=[["b1", "b2"]], line=[], want="k16"),
    "decon_onto_the_index": dict(old="A_k16", steps=[[]], line=[], decon=True, inplace=True, want="A_k16", want_decon="decon_only"),
    "append_and_decon": dict(old="A_k16", steps=[["b"]], line=[], decon=True, want="k16", want_decon="append_decon"),
    # (here the recorded result is the reference's FRESH build of a + b: its own append onto a direct-address index crashes)
    "direct_address": dict(old="A_k10", steps=[["b"]], line=[], want="k10", fresh_is_the_oracle=True),
}
RECORDED = ("k16", "k12", "TG", "none", "k10")          # the appended indexes the fixture holds, beside the old ones
# command lines that end before an index is read: first line of the reference's stderr and its status are recorded in cli.tsv
CLI_CASES = [["-t_db", "x"], ["-t_db", "x", "-o", "y"], ["-deCon", "c.fsa"], ["-deCon", "c.fsa", "-o", "y"]]

_COMP = str.maketrans("ACGTN", "TGCAN")


def fasta(part):
    return os.path.join(GOLDEN, part + ".fsa.gz")


def unpack(name, dst, tag="ref_"):
    """a stored index (name.comp.b.xz, name.length.b, name.name, name.seq.b) into folder dst -> its prefix"""
    prefix = os.path.join(str(dst), tag + name)
    put_xz(os.path.join(GOLDEN, name + ".comp.b.xz"), prefix + ".comp.b")
    for ext in (".length.b", ".name", ".seq.b"):
        with open(os.path.join(GOLDEN, name + ext), "rb") as f, open(prefix + ext, "wb") as g:
            g.write(f.read())
    return prefix


def put_xz(src, dst):
    with lzma.open(src, "rb") as f, open(dst, "wb") as g:
        g.write(f.read())
    return dst


def unpack_decon(name, dst):
    """a stored decontamination table (name.decon.comp.b.xz) into folder dst -> its path"""
    return put_xz(os.path.join(GOLDEN, name + ".decon.comp.b.xz"), os.path.join(str(dst), "ref_" + name + ".decon.comp.b"))


def cli_lines():
    """[(arguments, status, first line of stderr)] as recorded"""
    out = []
    for row in open(os.path.join(GOLDEN, "cli.tsv")).read().split("\n")[:-1]:
        args, status, line = row.split("\t")
        out.append((args.split(" "), int(status), line))
    return out


class Comp:
    """a .comp.b of either form (hashed, or direct-address: exist[] holds one entry per possible k-mer, 1 = none): the header, and
    keys / vidx / values with one entry per stored k-mer"""

    def __init__(self, path):
        b = open(path, "rb").read()
        self.DB_size, self.mlen, self.prefix_len = struct.unpack_from("<3I", b, 0)
        self.prefix, self.size, self.n, self.v_index, self.null_index = struct.unpack_from("<5Q", b, 12)
        self.mega = self.size == 1 << (2 * self.mlen)
        vdt = np.uint16 if self.DB_size < 65535 else np.uint32
        o = 52
        if self.mega:
            exist = np.frombuffer(b, np.uint32, self.size, o); o += 4 * self.size
            self.values = np.frombuffer(b, vdt, self.v_index, o); o += self.values.nbytes
            self.keys = np.nonzero(exist != 1)[0].astype(np.uint32)
            self.vidx = exist[self.keys]
        else:
            o += 4 * self.size
            self.values = np.frombuffer(b, vdt, self.v_index, o); o += self.values.nbytes
            self.keys = np.frombuffer(b, np.uint32, self.n, o); o += 4 * (self.n + 1)
            self.vidx = np.frombuffer(b, np.uint32, self.n, o); o += 4 * self.n
        self.kmersize, self.flag = struct.unpack_from("<2I", b, o)
        assert len(self.keys) == self.n and o + 8 == len(b), path

    def header(self):
        return (self.DB_size, self.mlen, self.kmersize, self.flag, self.n, self.prefix_len, self.prefix)

    def mapping(self):
        """{k-mer: tuple of ids}"""
        v = self.values.astype(np.int64).tolist()
        return {int(key): tuple(v[vi + 1:vi + 1 + v[vi]]) for key, vi in zip(self.keys.tolist(), self.vidx.tolist())}

    def stored_lists(self):
        """the lists as the value array holds them, each once: [tuple of ids]"""
        v = self.values.astype(np.int64).tolist()
        return [tuple(v[vi + 1:vi + 1 + v[vi]]) for vi in sorted(set(self.vidx.tolist()))]


def expand(comp_path):
    """the (k-mer << 32 | template) pairs a .comp.b holds, ascending, uint64: what the device's expansion is compared with"""
    c = comp_path if isinstance(comp_path, Comp) else Comp(comp_path)
    v = c.values.astype(np.int64)
    vi = c.vidx.astype(np.int64)
    cnt = v[vi]
    key = np.repeat(c.keys.astype(np.uint64), cnt)
    start = np.repeat(vi + 1, cnt)
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ids = v[start + within].astype(np.uint64)
    return np.sort((key << np.uint64(32)) | ids)


def _records(path):
    """[(sequence over ACGTN, untrimmed)] of a FASTA file, letters folded as the reference's table folds them"""
    raw = (gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")).read().decode("latin-1")
    return ["".join(siu._LETTERS.get(ch, "") for ch in rec.partition("\n")[2]) for rec in raw.split(">")[1:]]


def plain_kmers(seq, k):
    """the N-free k-mers of the forward strand (strings), repeats and all"""
    return [seq[j:j + k] for j in range(len(seq) - k + 1) if "N" not in seq[j:j + k]]


class Appended:
    """what the rule makes of an old index (files under prefix `old`) and new FASTA files: DB_size, k, prefix_len, prefix, lists
    (k-mer -> ascending ids), names, lengths (and slengths, ulengths of a sparse index) with slot 0 as the old file holds it, the new
    templates' sequences; with decon files also decon_lists (the pseudo-template DB_size behind the lists of the k-mers they hold)"""

    def __init__(self, old, paths, decon=()):
        c = Comp(old + ".comp.b")
        self.k, self.prefix_len, self.prefix = c.mlen, c.prefix_len, c.prefix
        self.sparse = not (c.prefix_len == 0 and c.prefix == 0)          # index.c:542-546
        text = ""
        for i in range(c.prefix_len):
            text = "ACGT"[(c.prefix >> (2 * i)) & 3] + text
        raw = np.fromfile(old + ".length.b", np.uint32)
        D = c.DB_size
        assert int(raw[0]) == D and len(raw) == 1 + (3 if self.sparse else 1) * D
        self.lengths = raw[1:1 + D].tolist()
        self.slengths = raw[1 + D:1 + 2 * D].tolist() if self.sparse else None
        self.ulengths = raw[1 + 2 * D:1 + 3 * D].tolist() if self.sparse else None
        self.names = open(old + ".name", "rb").read().decode("latin-1").split("\n")[:-1]
        assert len(self.names) == D - 1
        self.old_seq = np.fromfile(old + ".seq.b", np.uint64)
        self.lists = {km: list(ids) for km, ids in c.mapping().items()}
        self.new_seqs, self.skipped = [], []
        for path in paths:
            for name, seq, lead in siu.read_fasta(path):
                if self.sparse:
                    ws = siu.windows(seq, self.k, text) if len(seq) >= self.k else []
                    if not (self.k < len(seq) and ws):          # MinLen = k, MinKlen = 1 (no -ML beside -t_db)
                        self.skipped.append(name)
                        continue
                else:
                    if len(seq) < self.k:
                        self.skipped.append(name)
                        continue
                    ws = plain_kmers(seq, self.k)
                tid = len(self.lengths)
                uniq = set(ws)
                for km in uniq:
                    self.lists.setdefault(siu.encode(km), []).append(tid)
                self.names.append(name + (" B%d" % lead if lead else ""))
                self.lengths.append(len(seq))
                if self.sparse:
                    self.slengths.append(len(ws)); self.ulengths.append(len(uniq))
                self.new_seqs.append(seq)
        self.DB_size = len(self.lengths)
        self.decon_lists = None
        if decon:
            marked = set()
            for path in decon:
                for seq in _records(path):
                    if len(seq) > self.k:          # decon.c:193: LONGER than k, N's and all
                        for s in (seq, seq.translate(_COMP)[::-1]):
                            marked.update(siu.encode(km) for km in plain_kmers(s, self.k))
            self.decon_lists = {km: tuple(ids) + ((self.DB_size,) if km in marked else ()) for km, ids in self.lists.items()}
        self.lists = {km: tuple(ids) for km, ids in self.lists.items()}

    def header(self):
        return (self.DB_size, self.k, self.k, 0, len(self.lists), self.prefix_len, self.prefix)

    def v_index(self, lists=None):
        return sum(len(x) + 1 for x in set((self.lists if lists is None else lists).values()))

    def length_b(self):
        arrays = (self.lengths, self.slengths, self.ulengths) if self.sparse else (self.lengths,)
        return struct.pack("<I", self.DB_size) + b"".join(np.array(a, np.uint32).tobytes() for a in arrays)

    def name_file(self):
        return "".join(n + "\n" for n in self.names).encode("latin-1")

    def new_seq_words(self):
        """per new template the words of .seq.b that carry bases (N as A)"""
        out = []
        for s in self.new_seqs:
            out.append([siu.encode(s[a:a + 32].replace("N", "A")) << (2 * (32 - len(s[a:a + 32]))) for a in range(0, len(s), 32)])
        return out


def held_to(got, want_prefix, want_decon=None):
    """an Appended against the reference's recorded files"""
    ref = Comp(want_prefix + ".comp.b")
    assert got.header() == ref.header()
    assert got.lists == ref.mapping()
    assert got.v_index() == ref.v_index
    assert got.length_b() == open(want_prefix + ".length.b", "rb").read()
    assert got.name_file() == open(want_prefix + ".name", "rb").read()
    words = np.fromfile(want_prefix + ".seq.b", np.uint64)
    lens = np.asarray(got.lengths[1:], np.int64)
    assert len(words) == int(((lens >> 5) + 1).sum())
    n_old = got.DB_size - 1 - len(got.new_seqs)
    o = int(((lens[:n_old] >> 5) + 1).sum())
    assert np.array_equal(words[:o], got.old_seq)
    for L, ws in zip(lens[n_old:].tolist(), got.new_seq_words()):
        assert words[o:o + len(ws)].tolist() == ws
        o += (L >> 5) + 1
    if want_decon:
        d = Comp(want_decon)
        assert d.header() == ref.header() and got.decon_lists == d.mapping() and got.v_index(got.decon_lists) == d.v_index
        assert any(ids[-1] == got.DB_size for ids in got.decon_lists.values())


def same_comp(got_path, ref_path):
    """two .comp.b files hold the same index: header fields, mapping, v_index (equal lists are stored once in both); the form
    (hashed, direct-address), the bucket layout and the order of the lists are each builder's own"""
    a, b = Comp(got_path), Comp(ref_path)
    assert a.header() == b.header()
    assert a.mapping() == b.mapping()
    assert a.v_index == b.v_index
    return a


def same_index(got, ref, seq=True):
    """the files under prefix `got` against the reference's under `ref` (the comparisons of test_sparse_index_gpu.same_index)"""
    for ext in (".length.b", ".name"):
        assert open(got + ext, "rb").read() == open(ref + ext, "rb").read(), ext
    a = same_comp(got + ".comp.b", ref + ".comp.b")
    if seq:
        lens = np.fromfile(ref + ".length.b", np.uint32)
        siu.seq_words_equal(got + ".seq.b", ref + ".seq.b", lens[2:1 + int(lens[0])])
    return a


def files_equal(a, b, exts=(".comp.b", ".length.b", ".name", ".seq.b")):
    for ext in exts:
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
