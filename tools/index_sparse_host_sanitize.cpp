// index_sparse_host_sanitize.cpp -- the host side of the sparse index build (kma_amd/csrc/index_host.h: prefix and -ML arithmetic, the
// FASTA parser with the strict length gate, id assignment over skipped templates, the writers of .length.b / .seq.b / .name over the
// templates that stayed) under the host's sanitizers, in a program of its own that never touches a device. The windows the device
// counts are counted here on the host, with the same arithmetic; the files are compared with the reference's recorded ones.
// With a third argument (tests/golden/homology) the serial part of homology reduction runs too (hom_resolve, hom_report_line,
// sparse_assign_ids over the kept mask): the pairs and the rows the device hands over are counted here by brute force, in the device's
// formulation (flags per pair whoever is kept; winners over the kept columns by count, first walk position, id), and the report and
// files are compared with the reference's recorded ones.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wno-unused-function
//       -o /tmp/index_sparse_host_sanitize tools/index_sparse_host_sanitize.cpp -lz          (one command line)
//   mkdir -p /tmp/ishs && /tmp/index_sparse_host_sanitize tests/golden/sparse_index /tmp/ishs tests/golden/homology
//   (prints "all clean"; a finding of the sanitizers ends it with their report)
#include "../kma_amd/csrc/index_host.h"
#include <stdarg.h>
#include <zlib.h>
#include <map>
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

// one case of tests/golden/homology: the device's two passes by brute force, then the host rule
int run_hom(const char *tag, int k, const char *prefix, int min_len, double hq, double ht, bool and_mode, const std::string &dir, const std::string &out) {
	static const RefTable T;
	SparseRule r; r.k = k; r.kmerindex = k;
	if(sparse_parse_prefix(prefix, T, r)) { printf("%s: %s\n", tag, g_err); return 1; }
	sparse_set_gates(min_len, r);
	HomRule hom; hom.homQ = hq; hom.homT = ht; hom.and_mode = and_mode;
	std::vector<Tmpl> tm; std::vector<uint8_t> codes;
	std::vector<uint8_t> raw = gunzip(dir + "/db.fsa.gz");
	if(sparse_parse_fasta(raw, "db.fsa.gz", T, r.MinLen, codes, tm)) { printf("%s: %s\n", tag, g_err); return 1; }
	const int w = r.prefix_len + k;
	const size_t n = tm.size();
	const uint64_t kmask = (1ull << (2 * k)) - 1;
	// per template: k-mer -> (repeats, first walk position)
	std::vector<std::map<uint64_t, std::pair<uint32_t, uint32_t>>> km(n);
	std::vector<uint32_t> slen(n, 0);
	for(size_t t = 0; t < n; ++t) {
		const int len = tm[t].len;
		for(int p = 0; p + w <= len; ++p) {
			uint64_t x = 0, y = 0; bool ok = true;
			for(int i = 0; i < w; ++i) { uint8_t c = codes[tm[t].at + p + i]; ok = ok && c < 4; x = (x << 2) | (c & 3); y |= (uint64_t) (3 - (c & 3)) << (2 * i); }
			if(!ok) continue;
			auto add = [&](uint64_t key, uint32_t at) {
				++slen[t];
				auto it = km[t].find(key);
				if(it == km[t].end()) km[t][key] = {1u, at};
				else { ++it->second.first; if(at < it->second.second) it->second.second = at; }
			};
			if(!r.prefix_len || (x >> (2 * k)) == r.prefix) add(x & kmask, (uint32_t) p);
			if(!r.prefix_len || (y >> (2 * k)) == r.prefix) add(y & kmask, (uint32_t) (len + (len - w - p)));
		}
	}
	struct Cell { uint32_t tot = 0, uniq = 0, first = 0xFFFFFFFFu; };
	auto cell = [&](size_t i, size_t j) {
		Cell c;
		for(const auto &e : km[i]) if(km[j].count(e.first)) { c.tot += e.second.first; ++c.uniq; if(e.second.second < c.first) c.first = e.second.second; }
		return c;
	};
	std::vector<uint32_t> pairs;
	for(size_t i = 1; i < n; ++i) {
		if(!hom_eligible(slen[i], r)) continue;
		for(size_t j = 0; j < i; ++j) {
			const Cell c = cell(i, j);
			if(!c.tot) continue;
			const bool fq = 1.0 * c.tot / slen[i] >= hq, ft = hom.mode() == 2 && 1.0 * c.uniq / km[j].size() >= ht;
			if(fq || ft) { pairs.push_back((uint32_t) i); pairs.push_back((uint32_t) (j << 2) | (uint32_t) fq | ((uint32_t) ft << 1)); }
		}
	}
	std::vector<uint8_t> kept;
	hom_resolve(slen, r, hom, pairs.data(), pairs.size() / 2, kept);
	std::vector<uint32_t> new_id;
	const uint32_t n_kept = sparse_assign_ids(tm, slen, r, new_id, &kept);
	const std::string base = out + "/" + tag;
	FILE *f = fopen((base + ".report.tsv").c_str(), "wb");
	if(!f) { printf("%s: cannot create the report\n", tag); return 1; }
	int bad = 0;
	for(size_t i = 0; i < n; ++i) {
		if(!hom_eligible(slen[i], r)) continue;
		uint32_t tot = 0, jq = 0, fq = 0, num = 0, den = 0, jt = 0, ftt = 0;
		for(size_t j = 0; j < i; ++j) {
			if(!kept[j]) continue;
			const Cell c = cell(i, j);
			if(!c.tot) continue;
			if(c.tot > tot || (c.tot == tot && c.first < fq)) { tot = c.tot; jq = (uint32_t) j + 1; fq = c.first; }
			const double v = 1.0 * c.uniq / km[j].size(), b = num ? 1.0 * num / den : 0.0;
			if(v > b || (v == b && c.first < ftt)) { num = c.uniq; den = (uint32_t) km[j].size(); jt = (uint32_t) j + 1; ftt = c.first; }
		}
		if(!hom_report_line(f, hom, tm[i].name.substr(0, tm[i].head).c_str(), new_id[i], tot, slen[i], jq ? new_id[jq - 1] : 0, num, den, jt ? new_id[jt - 1] : 0)) {
			printf("%s: template %zu: the ratios contradict the flags\n", tag, i); bad = 1;
		}
	}
	fclose(f);
	std::vector<uint32_t> ulen(n_kept + 1, 0);
	for(size_t t = 0; t < n; ++t) if(new_id[t]) ulen[new_id[t]] = (uint32_t) km[t].size();
	if(n_kept && (sparse_write_length_b(base + ".length.b", tm, new_id, n_kept + 1, r.kmerindex, slen, ulen) || sparse_write_seq_and_names(base, tm, new_id, codes))) { printf("%s: %s\n", tag, g_err); return 1; }
	for(const char *ext : {".report.tsv", ".length.b", ".name"}) {
		if(slurp(base + ext) != slurp(dir + "/" + tag + ext)) { printf("%s%s differs from the reference's\n", tag, ext); bad = 1; }
	}
	printf("%s: %zu parsed, %u kept, %zu pairs, report and files %s\n", tag, n, n_kept, pairs.size() / 2, bad ? "DIFFER" : "equal");
	return bad;
}

int main(int argc, char **argv) {
	if(argc < 3) { fprintf(stderr, "usage: %s <tests/golden/sparse_index> <output folder>\n", argv[0]); return 2; }
	const std::string dir = argv[1], out = argv[2];
	int bad = run("k16_TG", 16, "TG", 0, dir, out) | run("k16_none", 16, "-", 0, dir, out) | run("k12_ATG", 12, "ATG", 0, dir, out) | run("k16_TG_ML60", 16, "TG", 60, dir, out);
	if(argc > 3) {
		const std::string hd = argv[3];
		for(const char *sp : {"TG", "-"}) {
			const std::string t = sp[0] == '-' ? "none" : "TG";
			bad |= run_hom((t + "_hq06").c_str(), 16, sp, 0, 0.6, 1.0, false, hd, out) | run_hom((t + "_hq05").c_str(), 16, sp, 0, 0.5, 1.0, false, hd, out) |
			       run_hom((t + "_ht045_hq045_and").c_str(), 16, sp, 0, 0.45, 0.45, true, hd, out) | run_hom((t + "_ht08_hq08").c_str(), 16, sp, 0, 0.8, 0.8, false, hd, out) |
			       run_hom((t + "_ht09").c_str(), 16, sp, 0, 1.0, 0.9, false, hd, out);
		}
		bad |= run_hom("TG_hq06_ML300", 16, "TG", 300, 0.6, 1.0, false, hd, out) | run_hom("k12_TG_hq06", 12, "TG", 0, 0.6, 1.0, false, hd, out) |
		       run_hom("k12_TG_ht08_hq08", 12, "TG", 0, 0.8, 0.8, false, hd, out);
	}
	static const RefTable T; SparseRule r;
	bad |= sparse_parse_prefix("", T, r) != KMAHIP_EINVAL || sparse_parse_prefix("TN", T, r) != KMAHIP_EINVAL || sparse_parse_prefix(nullptr, T, r) != KMAHIP_EINVAL ||
	       sparse_parse_prefix("TTTTTTTTTTTTTTTTT", T, r) != KMAHIP_EINVAL || sparse_parse_prefix("TTTTTTTTTTTTTTTT", T, r) != KMAHIP_OK;
	r.k = 16; r.kmerindex = 16; r.prefix_len = 0; sparse_set_gates(0x7FFFFFFF, r);
	printf("gates at INT_MAX: MinLen %d MinKlen %lld\n", r.MinLen, (long long) r.MinKlen);
	printf(bad ? "FAILED\n" : "all clean\n");
	return bad;
}
