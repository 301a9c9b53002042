// index_host_sanitize.cpp -- the index builder's host pass and file writer (write_comp_b, kma_amd/csrc/index.hip) under the host's
// sanitizers, in a program of its own that never touches a device: sorted (k-mer << 32 | template) pairs made here, with and without
// the keys of the pseudo-template of -deCon, written as .comp.b / .decon.comp.b and read back.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o /tmp/index_host_sanitize tools/index_host_sanitize.cpp -lz
//   /tmp/index_host_sanitize /tmp/ihs        (prints "ok"; a finding of the sanitizers ends it with their report)
#include "../kma_amd/csrc/index.hip"
#include <cstdarg>
#include <cstdio>
#include <random>

void kmahip_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
// what index.hip calls in other files of the library (the homology counts, the reader of .comp.b): never reached from here
int kmahip_hom_open(const unsigned long long *, int64_t, const int64_t *, const std::vector<uint32_t> &, int, int64_t, KmaHom **) { return KMAHIP_EDEVICE; }
int kmahip_hom_pairs(KmaHom *, double, double, bool, std::vector<KmaHomPair> &) { return KMAHIP_EDEVICE; }
int kmahip_hom_best(KmaHom *, const std::vector<uint8_t> &, std::vector<KmaHomRow> &) { return KMAHIP_EDEVICE; }
void kmahip_hom_close(KmaHom *) {}
int kmahip_comp_read(const std::string &, bool, KmaComp *) { return KMAHIP_EIO; }

static bool read_file(const std::string &path, std::vector<uint8_t> &buf) {
	FILE *f = fopen(path.c_str(), "rb");
	if(!f) return false;
	fseek(f, 0, SEEK_END); buf.resize((size_t) ftell(f)); fseek(f, 0, SEEK_SET);
	const bool ok = fread(buf.data(), 1, buf.size(), f) == buf.size();
	fclose(f);
	return ok;
}

// k-mers of the file that list template `id`
static size_t count_with(const std::vector<uint8_t> &b, uint32_t id, bool u16) {
	uint64_t h64[5];
	memcpy(h64, b.data() + 12, 40);
	const uint64_t size = h64[1], n = h64[2], v_index = h64[3];
	const uint8_t *values = b.data() + 52 + size * 4;
	const uint8_t *vidx = values + v_index * (u16 ? 2 : 4) + (n + 1) * 4;
	size_t c = 0;
	for(uint64_t i = 0; i < n; ++i) {
		uint32_t vi; memcpy(&vi, vidx + i * 4, 4);
		auto at = [&](uint64_t x) -> uint32_t { if(u16) { uint16_t v; memcpy(&v, values + x * 2, 2); return v; } uint32_t v; memcpy(&v, values + x * 4, 4); return v; };
		const uint32_t cnt = at(vi);
		for(uint32_t j = 1; j <= cnt; ++j) c += at(vi + j) == id;
	}
	return c;
}

int main(int argc, char **argv) {
	const std::string base = argc > 1 ? argv[1] : "/tmp/index_host_sanitize";
	for(uint32_t DB_size : {7u, 70000u}) {          // 16-bit and 32-bit value lists
		const int k = 12;
		std::mt19937_64 rng(DB_size);
		std::vector<unsigned long long> pairs;
		size_t marked = 0, only = 0;
		for(uint32_t km = 0; km < 50000; km += 1 + rng() % 5) {
			const int kind = (int) (rng() % 4);          // 0: templates only, 1: templates + contamination, 2: contamination only, 3: one template
			if(kind != 2) for(uint32_t t = 1 + rng() % 3; t < DB_size && t < 40; t += 1 + rng() % 9) { pairs.push_back(((unsigned long long) km << 32) | t); if(kind == 3) break; }
			if(kind == 1 || kind == 2) pairs.push_back(((unsigned long long) km << 32) | DB_size);
			marked += kind == 1; only += kind == 2;
		}
		if(write_comp_b(pairs, DB_size, k, false, base + ".comp.b") || write_comp_b(pairs, DB_size, k, true, base + ".decon.comp.b")) return 1;
		std::vector<uint8_t> a, b;
		if(!read_file(base + ".comp.b", a) || !read_file(base + ".decon.comp.b", b)) return 1;
		uint64_t na, nb;
		memcpy(&na, a.data() + 12 + 16, 8); memcpy(&nb, b.data() + 12 + 16, 8);
		const bool u16 = DB_size < 65535;
		if(na != nb || count_with(a, DB_size, u16) != 0 || count_with(b, DB_size, u16) != marked || only == 0) { fprintf(stderr, "mismatch at DB_size %u\n", DB_size); return 1; }
		// nothing but the pseudo-template: no k-mer at all
		std::vector<unsigned long long> lone(1, (7ull << 32) | DB_size);
		if(write_comp_b(lone, DB_size, k, true, base + ".none.comp.b") != KMAHIP_EFORMAT) return 1;
	}
	puts("ok");
	return 0;
}
