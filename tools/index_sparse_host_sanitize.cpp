// index_sparse_host_sanitize.cpp -- the host side of the sparse index build (kma_amd/csrc/index_host.h: prefix and -ML arithmetic, the
// FASTA parser with the strict length gate, id assignment over skipped templates, the writers of .length.b / .seq.b / .name over the
// templates that stayed) under the host's sanitizers, in a program of its own that never touches a device. The windows the device
// counts are counted here on the host, with the same arithmetic; the files are compared with the reference's recorded ones.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wno-unused-function
//       -o /tmp/index_sparse_host_sanitize tools/index_sparse_host_sanitize.cpp -lz          (one command line)
//   mkdir -p /tmp/ishs && /tmp/index_sparse_host_sanitize tests/golden/sparse_index /tmp/ishs
//   (prints "all clean"; a finding of the sanitizers ends it with their report)
#include "../kma_amd/csrc/index_host.h"
#include <stdarg.h>
#include <zlib.h>
#include <set>
#include <fstream>
#include <iterator>

static char g_err[512];
void kmahip_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }

static std::vector<uint8_t> slurp(const std::string &p) {
	std::ifstream f(p, std::ios::binary);
	return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static std::vector<uint8_t> gunzip(const std::string &p) {
	std::vector<uint8_t> out;
	gzFile f = gzopen(p.c_str(), "rb");
	if(!f) return out;
	uint8_t buf[4096];
	for(int got; (got = gzread(f, buf, sizeof buf)) > 0;) out.insert(out.end(), buf, buf + got);
	gzclose(f);
	return out;
}

int run(const char *tag, int k, const char *prefix, int min_len, const std::string &dir, const std::string &out) {
	static const RefTable T;
	SparseRule r; r.k = k; r.kmerindex = k;
	if(sparse_parse_prefix(prefix, T, r)) { printf("%s: %s\n", tag, g_err); return 1; }
	sparse_set_gates(min_len, r);
	std::vector<Tmpl> tm; std::vector<uint8_t> codes;
	for(const char *f : {"db1.fsa.gz", "db2.fsa.gz"}) {
		std::vector<uint8_t> raw = gunzip(dir + "/" + f);
		if(sparse_parse_fasta(raw, f, T, r.MinLen, codes, tm)) { printf("%s: %s\n", tag, g_err); return 1; }
	}
	const int w = r.prefix_len + k;
	std::vector<uint32_t> slen(tm.size(), 0);
	std::vector<std::set<uint64_t>> sets(tm.size());
	for(size_t t = 0; t < tm.size(); ++t) {
		for(int p = 0; p + w <= tm[t].len; ++p) {
			uint64_t x = 0, y = 0; bool ok = true;
			for(int i = 0; i < w; ++i) { uint8_t c = codes[tm[t].at + p + i]; ok = ok && c < 4; x = (x << 2) | (c & 3); y |= (uint64_t) (3 - (c & 3)) << (2 * i); }
			if(!ok) continue;
			const uint64_t kmask = (1ull << (2 * k)) - 1;
			if(!r.prefix_len || (x >> (2 * k)) == r.prefix) { ++slen[t]; sets[t].insert(x & kmask); }
			if(!r.prefix_len || (y >> (2 * k)) == r.prefix) { ++slen[t]; sets[t].insert(y & kmask); }
		}
	}
	std::vector<uint32_t> new_id;
	const uint32_t kept = sparse_assign_ids(tm, slen, r, new_id);
	std::vector<uint32_t> ulen(kept + 1, 0);
	for(size_t t = 0; t < tm.size(); ++t) if(new_id[t]) ulen[new_id[t]] = (uint32_t) sets[t].size();
	const std::string base = out + "/" + tag;
	if(sparse_write_length_b(base + ".length.b", tm, new_id, kept + 1, r.kmerindex, slen, ulen) || sparse_write_seq_and_names(base, tm, new_id, codes)) { printf("%s: %s\n", tag, g_err); return 1; }
	int bad = 0;
	for(const char *ext : {".length.b", ".name"}) {
		if(slurp(base + ext) != slurp(dir + "/" + tag + ext)) { printf("%s%s differs from the reference's\n", tag, ext); bad = 1; }
	}
	printf("%s: %zu parsed, %u kept, files %s\n", tag, tm.size(), kept, bad ? "DIFFER" : "equal");
	return bad;
}

int main(int argc, char **argv) {
	if(argc < 3) { fprintf(stderr, "usage: %s <tests/golden/sparse_index> <output folder>\n", argv[0]); return 2; }
	const std::string dir = argv[1], out = argv[2];
	int bad = run("k16_TG", 16, "TG", 0, dir, out) | run("k16_none", 16, "-", 0, dir, out) | run("k12_ATG", 12, "ATG", 0, dir, out) | run("k16_TG_ML60", 16, "TG", 60, dir, out);
	static const RefTable T; SparseRule r;
	bad |= sparse_parse_prefix("", T, r) != KMAHIP_EINVAL || sparse_parse_prefix("TN", T, r) != KMAHIP_EINVAL || sparse_parse_prefix(nullptr, T, r) != KMAHIP_EINVAL ||
	       sparse_parse_prefix("TTTTTTTTTTTTTTTTT", T, r) != KMAHIP_EINVAL || sparse_parse_prefix("TTTTTTTTTTTTTTTT", T, r) != KMAHIP_OK;
	r.k = 16; r.kmerindex = 16; r.prefix_len = 0; sparse_set_gates(0x7FFFFFFF, r);
	printf("gates at INT_MAX: MinLen %d MinKlen %lld\n", r.MinLen, (long long) r.MinKlen);
	printf(bad ? "FAILED\n" : "all clean\n");
	return bad;
}
