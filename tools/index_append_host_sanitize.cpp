// index_append_host_sanitize.cpp -- the host side of an append (`kmahip_index -t_db`; kma_amd/csrc/index_host.h: the check of the old
// index's value lists, the readers of .length.b / .name / .seq.b with their size checks and the clearing of the bits behind a
// template's last base, the writers over old content plus new templates, and the renaming at the end) under the host's sanitizers, in
// a program of its own that never touches a device. The new templates' windows are counted here on the host with the device's
// arithmetic; the files are compared with the reference's recorded ones. Then the checks are held to broken copies of the index:
// a list that starts or ends behind the value array, an empty one, an id of DB_size, a descending list, a k-mer wider than 2 k bits,
// a short .length.b, a .name with a line too few, a .seq.b a word short.
//
//   python3 -c "import sys; sys.path.insert(0, 'tests'); import index_append_util as u; [u.unpack(n, '/tmp/iahs') for n in list(u.OLD) + list(u.RECORDED)]"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wno-unused-function
//       -o /tmp/index_append_host_sanitize tools/index_append_host_sanitize.cpp -lz          (one command line; mkdir /tmp/iahs first)
//   /tmp/index_append_host_sanitize /tmp/iahs tests/golden/index_append
//   (prints "all clean"; a finding of the sanitizers ends it with their report)
#include "../kma_amd/csrc/index_host.h"
#include <stdarg.h>
#include <zlib.h>
#include <set>

static char g_err[512];
void kmahip_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }

static std::vector<uint8_t> gunzip(const std::string &p) {
	std::vector<uint8_t> out;
	gzFile f = gzopen(p.c_str(), "rb");
	if(!f) return out;
	uint8_t buf[4096];
	for(int got; (got = gzread(f, buf, sizeof buf)) > 0;) out.insert(out.end(), buf, buf + got);
	gzclose(f);
	return out;
}

// .comp.b of either form into keys / vidx / values, as kmahip_comp_read hands them on
struct Comp {
	uint32_t DB_size = 0, mlen = 0, prefix_len = 0;
	uint64_t prefix = 0, size = 0, n = 0, v_index = 0;
	bool u16 = false;
	std::vector<uint8_t> values;
	std::vector<uint32_t> keys, vidx;
};

static bool read_comp(const std::string &path, Comp &c) {
	std::vector<uint8_t> b;
	if(!append_slurp(path, b) || b.size() < 60) return false;
	uint64_t h64[5];
	memcpy(&c.DB_size, b.data(), 4); memcpy(&c.mlen, b.data() + 4, 4); memcpy(&c.prefix_len, b.data() + 8, 4); memcpy(h64, b.data() + 12, 40);
	c.prefix = h64[0]; c.size = h64[1]; c.n = h64[2]; c.v_index = h64[3];
	c.u16 = c.DB_size < 65535;
	const size_t vbytes = (size_t) c.v_index * (c.u16 ? 2 : 4);
	size_t o = 52;
	if(c.size == 1ull << (2 * c.mlen)) {
		if(o + 4 * c.size + vbytes > b.size()) return false;
		for(uint64_t i = 0; i < c.size; ++i) { uint32_t e; memcpy(&e, b.data() + o + 4 * i, 4); if(e != 1) { c.keys.push_back((uint32_t) i); c.vidx.push_back(e); } }
		o += 4 * c.size;
		c.values.assign(b.begin() + o, b.begin() + o + vbytes);
		c.n = c.keys.size();
	} else {
		o += 4 * c.size;
		if(o + vbytes + 4 * (2 * c.n + 1) > b.size()) return false;
		c.values.assign(b.begin() + o, b.begin() + o + vbytes); o += vbytes;
		c.keys.resize(c.n); c.vidx.resize(c.n);
		memcpy(c.keys.data(), b.data() + o, 4 * c.n); o += 4 * (c.n + 1);
		memcpy(c.vidx.data(), b.data() + o, 4 * c.n);
	}
	return true;
}

static int check(const Comp &c, uint64_t *pairs) {
	return append_check_lists(c.keys.data(), c.vidx.data(), c.n, c.values.data(), c.u16, c.v_index, c.DB_size, (int) c.mlen, pairs);
}

// one append on the host: old index `old_name` plus b.fsa.gz -> the files under out/<tag>, held to the recorded ones under dir/<want>
static int run(const char *tag, const char *old_name, const char *want, const std::string &dir, const std::string &golden) {
	static const RefTable T;
	Comp c;
	const std::string old = dir + "/ref_" + old_name, base = dir + "/" + tag, tmp = base + ".appending";
	if(!read_comp(old + ".comp.b", c)) { printf("%s: cannot read %s.comp.b\n", tag, old.c_str()); return 1; }
	uint64_t n_pairs = 0;
	if(check(c, &n_pairs)) { printf("%s: %s\n", tag, g_err); return 1; }
	const bool sparse = !(c.prefix_len == 0 && c.prefix == 0);
	OldAnnots ann;
	if(append_read_annots(old, c.DB_size, sparse, true, ann)) { printf("%s: %s\n", tag, g_err); return 1; }
	const int k = (int) c.mlen;
	SparseRule r; r.k = k; r.kmerindex = k; r.prefix_len = (int) c.prefix_len; r.prefix = c.prefix;
	sparse_set_gates(0, r);
	std::vector<Tmpl> tm; std::vector<uint8_t> codes;
	const std::vector<uint8_t> raw = gunzip(golden + "/b.fsa.gz");
	if(sparse_parse_fasta(raw, "b.fsa.gz", T, sparse ? r.MinLen : k - 1, codes, tm)) { printf("%s: %s\n", tag, g_err); return 1; }
	const int w = r.prefix_len + k;
	const uint64_t kmask = (1ull << (2 * k)) - 1;
	std::vector<uint32_t> slen(tm.size(), 0), new_id;
	std::vector<std::set<uint64_t>> sets(tm.size());
	for(size_t t = 0; sparse && t < tm.size(); ++t) {
		for(int p = 0; p + w <= tm[t].len; ++p) {
			uint64_t x = 0, y = 0; bool ok = true;
			for(int i = 0; i < w; ++i) { const uint8_t ch = codes[tm[t].at + p + i]; ok = ok && ch < 4; x = (x << 2) | (ch & 3); y |= (uint64_t) (3 - (ch & 3)) << (2 * i); }
			if(!ok) continue;
			if(!r.prefix_len || (x >> (2 * k)) == r.prefix) { ++slen[t]; sets[t].insert(x & kmask); }
			if(!r.prefix_len || (y >> (2 * k)) == r.prefix) { ++slen[t]; sets[t].insert(y & kmask); }
		}
	}
	if(sparse) sparse_assign_ids(tm, slen, r, new_id);
	else { new_id.resize(tm.size()); for(size_t t = 0; t < tm.size(); ++t) new_id[t] = (uint32_t) t + 1; }
	uint32_t DB_size = c.DB_size;
	for(uint32_t &id : new_id) if(id) { id += c.DB_size - 1; DB_size = id + 1; }
	std::vector<uint32_t> lens(ann.lens), sl(ann.slen), ul(ann.ulen);
	lens.resize(DB_size, 0);
	if(sparse) { sl.resize(DB_size, 0); ul.resize(DB_size, 0); }
	for(size_t t = 0; t < tm.size(); ++t) {
		if(!new_id[t]) continue;
		lens[new_id[t]] = (uint32_t) tm[t].len;
		if(sparse) { sl[new_id[t]] = slen[t]; ul[new_id[t]] = (uint32_t) sets[t].size(); }
	}
	if(append_write_length_b(tmp + ".length.b", DB_size, lens, sparse ? &sl : nullptr, sparse ? &ul : nullptr) ||
	   sparse_write_seq_and_names(tmp, tm, new_id, codes, &ann.seq, &ann.names) ||
	   append_commit(tmp, base, {".length.b", ".seq.b", ".name"}, true)) { printf("%s: %s\n", tag, g_err); return 1; }
	int bad = 0;
	std::vector<uint8_t> a, b;
	for(const char *ext : {".length.b", ".name"}) {
		if(!append_slurp(base + ext, a) || !append_slurp(dir + "/ref_" + want + ext, b) || a != b) { printf("%s%s differs from the reference's\n", tag, ext); bad = 1; }
	}
	// .seq.b: the words that carry bases (behind a length that is a multiple of 32 the reference's word is what its buffer held)
	if(!append_slurp(base + ".seq.b", a) || !append_slurp(dir + "/ref_" + want + ".seq.b", b) || a.size() != b.size()) { printf("%s.seq.b: another size than the reference's\n", tag); bad = 1; }
	else {
		size_t o = 0;
		for(uint32_t t = 1; t < DB_size; ++t) {
			const size_t carry = ((size_t) lens[t] + 31) >> 5;
			if(memcmp(a.data() + 8 * o, b.data() + 8 * o, 8 * carry)) { printf("%s.seq.b differs in template %u\n", tag, t); bad = 1; }
			o += ((size_t) lens[t] >> 5) + 1;
		}
		if(8 * o != a.size()) { printf("%s.seq.b: %zu words for %zu bytes\n", tag, o, a.size()); bad = 1; }
	}
	FILE *left = fopen((tmp + ".length.b").c_str(), "rb");
	if(left) { fclose(left); printf("%s: a temporary file is left\n", tag); bad = 1; }
	printf("%s: %llu old pairs, %zu new templates, DB_size %u, files %s\n", tag, (unsigned long long) n_pairs, tm.size(), DB_size, bad ? "DIFFER" : "equal");
	return bad;
}

static void put32(std::vector<uint8_t> &v, bool u16, uint64_t at, uint32_t x) {
	if(u16) { const uint16_t y = (uint16_t) x; memcpy(v.data() + 2 * at, &y, 2); } else memcpy(v.data() + 4 * at, &x, 4);
}

static uint32_t get32(const std::vector<uint8_t> &v, bool u16, uint64_t at) {
	if(u16) { uint16_t y; memcpy(&y, v.data() + 2 * at, 2); return y; }
	uint32_t x; memcpy(&x, v.data() + 4 * at, 4); return x;
}

// every way a file can contradict its header: KMAHIP_EFORMAT and the reference's words, nothing read out of bounds
static int broken(const std::string &dir) {
	Comp good;
	if(!read_comp(dir + "/ref_A_k16.comp.b", good)) return 1;
	int bad = 0;
	uint64_t pairs = 0;
	auto refused = [&](const Comp &c, const char *what) {
		g_err[0] = 0;
		const int rc = check(c, &pairs);
		if(rc != KMAHIP_EFORMAT || !strstr(g_err, KMAHIP_WRONG_DB)) { printf("not refused: %s (%d, %s)\n", what, rc, g_err); bad = 1; }
	};
	// a k-mer with a list of two ids at least, for the order check
	size_t two = 0;
	while(two < good.n && get32(good.values, good.u16, good.vidx[two]) < 2) ++two;
	if(two == good.n) { printf("no list of two ids\n"); return 1; }
	{ Comp c = good; c.vidx[5] = (uint32_t) c.v_index; refused(c, "a list that starts at v_index"); }
	{ Comp c = good; c.vidx[5] = 0xFFFFFFFFu; refused(c, "a list that starts at 2^32 - 1"); }
	{ Comp c = good; put32(c.values, c.u16, c.vidx[5], 0); refused(c, "an empty list"); }
	{ Comp c = good; c.vidx[5] = (uint32_t) c.v_index - 1; put32(c.values, c.u16, c.v_index - 1, 3); refused(c, "a list that ends behind v_index"); }
	{ Comp c = good; put32(c.values, c.u16, (uint64_t) c.vidx[5] + 1, c.DB_size); refused(c, "an id of DB_size"); }
	{ Comp c = good; put32(c.values, c.u16, (uint64_t) c.vidx[5] + 1, 0); refused(c, "an id of 0"); }
	{ Comp c = good; const uint64_t at = c.vidx[two]; const uint32_t x = get32(c.values, c.u16, at + 1); put32(c.values, c.u16, at + 1, get32(c.values, c.u16, at + 2)); put32(c.values, c.u16, at + 2, x); refused(c, "a descending list"); }
	{ Comp c = good; c.mlen = 12; refused(c, "a k-mer wider than 2 k bits"); }
	{ Comp c = good; c.DB_size = 1; refused(c, "no template"); }
	if(check(good, &pairs)) { printf("the index as it is: %s\n", g_err); bad = 1; }
	// the annotation files
	const std::string base = dir + "/broken";
	std::vector<uint8_t> len_b, names, seq;
	append_slurp(dir + "/ref_A_k16.length.b", len_b); append_slurp(dir + "/ref_A_k16.name", names); append_slurp(dir + "/ref_A_k16.seq.b", seq);
	auto write = [&](const char *ext, const std::vector<uint8_t> &v, size_t n) { FILE *f = fopen((base + ext).c_str(), "wb"); fwrite(v.data(), 1, n, f); fclose(f); };
	auto annots_refused = [&](const char *what, bool sparse) {
		OldAnnots a; g_err[0] = 0;
		const int rc = append_read_annots(base, good.DB_size, sparse, true, a);
		if(rc != KMAHIP_EFORMAT || !strstr(g_err, KMAHIP_WRONG_DB)) { printf("not refused: %s (%d, %s)\n", what, rc, g_err); bad = 1; }
	};
	write(".length.b", len_b, len_b.size() - 4); write(".name", names, names.size()); write(".seq.b", seq, seq.size());
	annots_refused("a .length.b a word short", false);
	write(".length.b", len_b, len_b.size());
	annots_refused("one array in .length.b where a sparse index has three", true);
	write(".name", names, names.size() - 1);
	annots_refused("a .name whose last line does not end", false);
	write(".name", names, names.size()); write(".seq.b", seq, seq.size() - 8);
	annots_refused("a .seq.b a word short", false);
	write(".seq.b", seq, seq.size());
	{ OldAnnots a; if(append_read_annots(base, good.DB_size, false, true, a)) { printf("the files as they are: %s\n", g_err); bad = 1; } }
	for(const char *ext : {".length.b", ".name", ".seq.b"}) remove((base + ext).c_str());
	printf("broken copies: %s\n", bad ? "NOT all refused" : "all refused");
	return bad;
}

int main(int argc, char **argv) {
	if(argc < 3) { fprintf(stderr, "usage: %s <folder with the unpacked fixture indexes> <tests/golden/index_append>\n", argv[0]); return 2; }
	const std::string dir = argv[1], golden = argv[2];
	int bad = run("k16", "A_k16", "k16", dir, golden) | run("k12", "A_k12", "k12", dir, golden) | run("TG", "A_TG", "TG", dir, golden) | run("none", "A_none", "none", dir, golden) |
	          run("k10", "A_k10", "k10", dir, golden);
	bad |= broken(dir);
	printf(bad ? "FAILED\n" : "all clean\n");
	return bad;
}
