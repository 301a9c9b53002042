// index_host.h -- the host side of a sparse index build (`kma index -Sparse`), free of any device call so that it also compiles into a
// plain C++ program: the letter table, the FASTA parser with the sparse build's length gate, the prefix and -ML arithmetic of
// index.c:451-474 / 576-613, the choice of the templates that stay (makeindex.c:225, updateindex.c:79-167, qualcheck.c:31-79) and
// the writers of .length.b / .seq.b / .name over the templates that stayed (updateAnnots_sparse, makeindex.c:262-276).
// With -hq / -ht (queryCheck, templateCheck, qualcheck.c:81-324) also the serial part of homology reduction: who stays, given the pairs
// the device flagged, and the line each template gets.
// With -t_db (kmahip_index_append) the host side of an append: the check of the old index's value lists before any of them reaches the
// device, the readers of its .length.b / .name / .seq.b, the writer of .length.b from whole arrays, and the renaming at the end.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <ctype.h>
#include <string>
#include <vector>
#include "../../include/kmahip.h"

void kmahip_set_error(const char *fmt, ...);

namespace {

struct Tmpl {
	std::string name;
	size_t at = 0;       // first base in the concatenated code array
	int len = 0;
	size_t head = 0;     // the bytes of name that are the record's header (" B<n>" may follow)
};

// index.c:128-170
struct RefTable {
	uint8_t t[256];
	RefTable() {
		memset(t, 8, sizeof t);
		t[(int) '\n'] = 16;
		const char *codes[5] = {"ARMDrmd", "CYBcyb", "GSKVgskv", "TWHUtwhu", "NXnx"};
		for(int c = 0; c < 5; ++c) for(const char *p = codes[c]; *p; ++p) t[(int) (unsigned char) *p] = (uint8_t) c;
		t[(int) 'a'] = 0;
	}
};

// what -Sparse, -k and -ML come to (index.c:451-474, 576-613)
struct SparseRule {
	int k = 16, kmerindex = 16;
	int prefix_len = 0;
	uint64_t prefix = 1;        // the header's value: 1 stands for "no prefix"
	int MinLen = 16;            // a template stays when MinLen < its length (lenCheck, makeindex.c:46-48)
	int64_t MinKlen = 1;        // ... and when its windows (no prefix: its k-mer starts, twice) reach MinKlen (lengthCheck)
};

// "-" = no prefix; anything else: letters the table maps to 0 ... 3, at least one and at most 16 of them
inline int sparse_parse_prefix(const char *text, const RefTable &T, SparseRule &r) {
	if(!text) { kmahip_set_error("sparse index: null prefix (\"-\" stands for none)"); return KMAHIP_EINVAL; }
	if(!strcmp(text, "-")) { r.prefix_len = 0; r.prefix = 1; return KMAHIP_OK; }
	const size_t n = strlen(text);
	if(n == 0) { kmahip_set_error("Invalid prefix."); return KMAHIP_EINVAL; }
	if(n > 16) { kmahip_set_error("sparse index: a prefix of %zu bases: at most 16 supported", n); return KMAHIP_EINVAL; }
	uint64_t p = 0;
	for(size_t i = 0; i < n; ++i) {
		const uint8_t c = T.t[(unsigned char) text[i]];
		if(c > 3) { kmahip_set_error("Invalid prefix."); return KMAHIP_EINVAL; }
		p = (p << 2) | c;
	}
	r.prefix_len = (int) n; r.prefix = p;
	return KMAHIP_OK;
}

// index.c:599-606; min_len <= 0: no -ML
inline void sparse_set_gates(int min_len, SparseRule &r) {
	if(min_len > r.k + r.prefix_len + 1) {
		r.MinLen = min_len;
		r.MinKlen = 2 * ((int64_t) min_len - r.k - r.prefix_len + 1);
		for(int i = 0; i < r.prefix_len; ++i) r.MinKlen /= 4;
	} else {
		r.MinLen = r.k > r.kmerindex ? r.k : r.kmerindex;
		r.MinKlen = 1;
	}
}

// One FASTA file already in memory -> its records behind `tm` / `codes`, as the plain build parses them (FileBuffgetFsa,
// seqparse.c:66-159; compDNAref, compdna.c:129-147), with the sparse build's gate: a record of min_len bases or fewer goes
int sparse_parse_fasta(const std::vector<uint8_t> &raw, const char *path, const RefTable &T, int min_len, std::vector<uint8_t> &codes, std::vector<Tmpl> &tm) {
	if(raw.empty() || raw[0] != '>') { kmahip_set_error("%s is not a FASTA file", path); return KMAHIP_EFORMAT; }
	size_t p = 0;
	while(p < raw.size()) {
		size_t e = p;
		while(e < raw.size() && raw[e] != '\n') ++e;
		size_t h = e;
		while(h > p + 1 && isspace(raw[h - 1])) --h;
		std::string name((const char *) raw.data() + p + 1, h - p - 1);
		p = e < raw.size() ? e + 1 : e;
		const size_t at = codes.size();
		while(p < raw.size() && raw[p] != '>') { const uint8_t c = T.t[raw[p]]; if(c < 8) codes.push_back(c); ++p; }
		size_t a = at, b = codes.size();
		while(a < b && codes[a] == 4) ++a;
		while(b > a && codes[b - 1] == 4) --b;
		const int bias = (int) (a - at);
		if(a > at) memmove(codes.data() + at, codes.data() + a, b - a);
		codes.resize(at + (b - a));
		const size_t len = b - a;
		if(len > 0x7FFFFFFFu) { kmahip_set_error("%s: a template of %zu bases", path, len); return KMAHIP_EFORMAT; }
		if(!((size_t) min_len < len)) { codes.resize(at); continue; }              // "# Skipped"
		const size_t head = name.size();
		if(bias > 0) name += " B" + std::to_string(bias);
		Tmpl t; t.name = name; t.at = at; t.len = (int) len; t.head = head;
		tm.push_back(t);
	}
	return KMAHIP_OK;
}

// The templates that stay, from their window counts over both strands (slen[t], t = 0 .. n_t - 1 in file order): lengthCheck asks
// for MinKlen windows (without a prefix: of (len - k + 1) * 2, whatever N's there are), update_DB for one at least. new_id[t] = the
// id of the template in the index, 1 .. , or 0 when it is skipped; every template behind a skipped one moves up. -> how many stay
// kept (a homology build, hom_resolve): the templates that stay are those it marks, which passed queryCheck's / templateCheck's gate
inline uint32_t sparse_assign_ids(const std::vector<Tmpl> &tm, const std::vector<uint32_t> &slen, const SparseRule &r, std::vector<uint32_t> &new_id,
                                  const std::vector<uint8_t> *kept = nullptr) {
	new_id.assign(tm.size(), 0);
	uint32_t next = 1;
	for(size_t t = 0; t < tm.size(); ++t) {
		if(kept) { if((*kept)[t]) new_id[t] = next++; continue; }
		const int64_t have = r.prefix_len ? (int64_t) slen[t] : ((int64_t) tm[t].len - r.k + 1) * 2;
		if(have < r.MinKlen || slen[t] == 0) continue;
		new_id[t] = next++;
	}
	return next - 1;
}

// ---- homology reduction: `-hq x -ht y [-and]` (index.c:309-350, 607-613; queryCheck / templateCheck, qualcheck.c:81-324) -------
// The reference scores a new template against the templates kept so far and keeps it when its best ratios stay below the thresholds.
// The device counts every pair (homology.hip); what is here is the serial part: who stays, and the line each template gets.
struct HomRule {
	double homQ = 1.0, homT = 1.0;
	bool and_mode = false;                  // cmp: OR by default, AND under -and
	int mode() const { return homT < 1 ? 2 : homQ < 1 ? 1 : 0; }          // 2 templateCheck, 1 queryCheck, 0 lengthCheck (index.c:607-613)
	// does a template stay whose best ratios are below the thresholds as given (qualcheck.c:181, :314)
	bool stays(bool q_below, bool t_below) const { return mode() == 1 ? q_below : and_mode ? (t_below && q_below) : (t_below || q_below); }
};

// queryCheck and templateCheck count the windows themselves, N's and all, with a prefix and without (thisKlen < MinKlen: no line, no id)
inline bool hom_eligible(uint32_t windows, const SparseRule &r) { return windows > 0 && (int64_t) windows >= r.MinKlen; }

// Who stays, in file order. pairs: n_pairs times (row, column * 4 + flags) in any order, the flags of a pair being 1: thisQ >= homQ,
// 2: thisT >= homT (every pair with a flag is there, whoever is kept). bestQ < homQ fails iff a kept column carries flag 1, bestT <
// homT iff one carries flag 2: the maxima need not be known. kept[t] = 1 for the templates that get an id
inline void hom_resolve(const std::vector<uint32_t> &slen, const SparseRule &r, const HomRule &hom, const uint32_t *pairs, size_t n_pairs, std::vector<uint8_t> &kept) {
	const size_t n_t = slen.size();
	std::vector<size_t> start(n_t + 1, 0);
	for(size_t p = 0; p < n_pairs; ++p) ++start[(size_t) pairs[2 * p] + 1];
	for(size_t t = 0; t < n_t; ++t) start[t + 1] += start[t];
	std::vector<uint32_t> by_row(n_pairs);
	{
		std::vector<size_t> at(start.begin(), start.end() - 1);
		for(size_t p = 0; p < n_pairs; ++p) by_row[at[pairs[2 * p]]++] = pairs[2 * p + 1];
	}
	kept.assign(n_t, 0);
	for(size_t t = 0; t < n_t; ++t) {
		if(!hom_eligible(slen[t], r)) continue;
		unsigned seen = 0;
		for(size_t p = start[t]; p < start[t + 1]; ++p) if(kept[by_row[p] >> 2]) seen |= by_row[p] & 3u;
		// (a maximum over no column is 0, which a threshold of 0 does not let pass: -hq 0 keeps nothing)
		kept[t] = hom.stays(!(seen & 1u) && 0 < hom.homQ, !(seen & 2u) && 0 < hom.homT);
	}
}

// The line of one template (qualcheck.c:182-186, :315-318) from the integers of its row: Scores_tot of templateQ over thisKlen, Scores
// over ulen of templateT; idQ, idT: the winners' ids in the index (0: none). id: the template's own id when it stays, else 0.
// -> whether the doubles formed here say the same as `id` (the device's flags and these ratios are one expression)
inline bool hom_report_line(FILE *f, const HomRule &hom, const char *name, uint32_t id, uint32_t tot, uint32_t klen, uint32_t idQ, uint32_t num, uint32_t den, uint32_t idT) {
	const double bestQ = tot ? 1.0 * tot / klen : 0.0, bestT = num ? 1.0 * num / den : 0.0;
	const bool stays = hom.stays(bestQ < hom.homQ, bestT < hom.homT);
	if(f) {
		if(hom.mode() == 1) fprintf(f, "%s\t%d\t%f\t%d\n", name, (int) (id ? id : idQ), bestQ, (int) idQ);
		else fprintf(f, "%s\t%d\t%f\t%d\t%f\t%d\n", name, (int) (id ? id : (bestT < hom.homT) ? idQ : idT), bestQ, (int) idQ, bestT, (int) idT);
	}
	return stays == (id != 0);
}

// .length.b of a sparse index (makeindex.c:262-270): DB_size, lengths (slot 0: kmerindex), slengths, ulengths (slot 0: 0).
// slen by template in file order, ulen by the id in the index (DB_size entries, as the device counted them)
int sparse_write_length_b(const std::string &path, const std::vector<Tmpl> &tm, const std::vector<uint32_t> &new_id, uint32_t DB_size, int kmerindex,
                          const std::vector<uint32_t> &slen, const std::vector<uint32_t> &ulen) {
	std::vector<uint32_t> out((size_t) 1 + 3 * (size_t) DB_size, 0);
	out[0] = DB_size;
	uint32_t *lens = out.data() + 1, *sl = lens + DB_size, *ul = sl + DB_size;
	lens[0] = (uint32_t) kmerindex;
	for(size_t t = 0; t < tm.size(); ++t) {
		const uint32_t id = new_id[t];
		if(!id) continue;
		lens[id] = (uint32_t) tm[t].len; sl[id] = slen[t]; ul[id] = ulen[id];
	}
	FILE *f = fopen(path.c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s", path.c_str()); return KMAHIP_EIO; }
	bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
	ok = (fclose(f) == 0) && ok;
	if(!ok) { kmahip_set_error("writing %s failed", path.c_str()); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

// .seq.b and .name over the templates that stayed: (len >> 5) + 1 words each, 32 bases a word from the top, N as A.
// old_seq, old_names (an append): what the index held before, written in front
int sparse_write_seq_and_names(const std::string &base, const std::vector<Tmpl> &tm, const std::vector<uint32_t> &new_id, const std::vector<uint8_t> &codes,
                               const std::vector<uint8_t> *old_seq = nullptr, const std::vector<uint8_t> *old_names = nullptr) {
	FILE *f = fopen((base + ".seq.b").c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s.seq.b", base.c_str()); return KMAHIP_EIO; }
	bool ok = true;
	if(old_seq && !old_seq->empty()) ok = fwrite(old_seq->data(), 1, old_seq->size(), f) == old_seq->size();
	std::vector<uint64_t> words;
	for(size_t t = 0; t < tm.size(); ++t) {
		if(!new_id[t]) continue;
		const Tmpl &x = tm[t];
		words.assign((size_t) (x.len >> 5) + 1, 0);
		for(int i = 0; i < x.len; ++i) words[(size_t) i >> 5] |= (uint64_t) (codes[x.at + (size_t) i] & 3) << (62 - ((i & 31) << 1));
		ok = fwrite(words.data(), 8, words.size(), f) == words.size() && ok;
	}
	ok = (fclose(f) == 0) && ok;
	f = fopen((base + ".name").c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s.name", base.c_str()); return KMAHIP_EIO; }
	if(old_names && !old_names->empty()) ok = fwrite(old_names->data(), 1, old_names->size(), f) == old_names->size() && ok;
	for(size_t t = 0; t < tm.size(); ++t) if(new_id[t]) ok = fprintf(f, "%s\n", tm[t].name.c_str()) > 0 && ok;
	ok = (fclose(f) == 0) && ok;
	if(!ok) { kmahip_set_error("writing the index under %s failed", base.c_str()); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

// ---- appending to an index: `kma index -t_db <prefix>` (index.c:221-229, 529-557, 616-674; load_DBs, loadupdate.c:151-210) -------
// The old index as an append needs it, apart from .comp.b (which kmahip_comp_read holds): the arrays of .length.b (one, or three
// for a sparse index), and the bytes of .name and .seq.b, which go in front of the new templates'.
struct OldAnnots {
	std::vector<uint32_t> lens, slen, ulen;          // DB_size entries each; slen, ulen: a sparse index alone
	std::vector<uint8_t> names, seq;
};

#define KMAHIP_WRONG_DB "Wrong format of DB."          // (what the reference says, loadupdate.c:163)

inline bool append_slurp(const std::string &path, std::vector<uint8_t> &buf) {
	FILE *f = fopen(path.c_str(), "rb");
	if(!f) return false;
	buf.clear();
	uint8_t chunk[1 << 16];
	for(size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
	const bool ok = !ferror(f);
	fclose(f);
	return ok;
}

// The value lists of an index before anything of it reaches the device: every list lies inside `values` (v_index elements of 2 or 4
// bytes: count, then the ids), holds at least one id, ascends, and names templates 1 .. DB_size - 1; every k-mer fits 2 k bits. Each
// list is walked once however many k-mers share it. *n_pairs = the (k-mer, template) pairs the index holds
inline int append_check_lists(const uint32_t *keys, const uint32_t *vidx, uint64_t n, const void *values, bool u16, uint64_t v_index, uint32_t DB_size, int k,
                              uint64_t *n_pairs) {
	const uint16_t *v16 = (const uint16_t *) values;
	const uint32_t *v32 = (const uint32_t *) values;
	const uint64_t kmask = (1ull << (2 * k)) - 1;
	std::vector<uint8_t> seen((size_t) v_index, 0);
	uint64_t total = 0;
	if(DB_size < 2 || n == 0) { kmahip_set_error(KMAHIP_WRONG_DB " (%u templates, %llu k-mers)", DB_size ? DB_size - 1 : 0, (unsigned long long) n); return KMAHIP_EFORMAT; }
	for(uint64_t i = 0; i < n; ++i) {
		const uint64_t at = vidx[i];
		if(keys[i] > kmask) { kmahip_set_error(KMAHIP_WRONG_DB " (k-mer %llu of %d bases: 0x%x)", (unsigned long long) i, k, keys[i]); return KMAHIP_EFORMAT; }
		if(at >= v_index) { kmahip_set_error(KMAHIP_WRONG_DB " (k-mer %llu: its list starts at %llu of %llu)", (unsigned long long) i, (unsigned long long) at, (unsigned long long) v_index); return KMAHIP_EFORMAT; }
		const uint64_t cnt = u16 ? v16[at] : v32[at];
		if(cnt == 0 || cnt >= DB_size || at + 1 + cnt > v_index) {
			kmahip_set_error(KMAHIP_WRONG_DB " (k-mer %llu: a list of %llu at %llu of %llu)", (unsigned long long) i, (unsigned long long) cnt, (unsigned long long) at, (unsigned long long) v_index);
			return KMAHIP_EFORMAT;
		}
		total += cnt;
		if(seen[(size_t) at]) continue;
		seen[(size_t) at] = 1;
		uint32_t last = 0;
		for(uint64_t j = at + 1; j <= at + cnt; ++j) {
			const uint32_t id = u16 ? v16[j] : v32[j];
			if(id <= last || id >= DB_size) { kmahip_set_error(KMAHIP_WRONG_DB " (k-mer %llu: template %u behind %u, %u in the index)", (unsigned long long) i, id, last, DB_size - 1); return KMAHIP_EFORMAT; }
			last = id;
		}
	}
	*n_pairs = total;
	return KMAHIP_OK;
}

// <prefix>.length.b, and with `all` <prefix>.name and .seq.b: sizes held against DB_size and the lengths. The words of .seq.b are
// brought to the form this builder writes: the bits behind a template's last base are 0 (where a length is a multiple of 32 the
// reference's last word is whatever its buffer held, updateindex.c:187), so an appended index does not depend on who built the old one
inline int append_read_annots(const std::string &base, uint32_t DB_size, bool sparse, bool all, OldAnnots &o) {
	std::vector<uint8_t> raw;
	if(!append_slurp(base + ".length.b", raw)) { kmahip_set_error("cannot read %s.length.b", base.c_str()); return KMAHIP_EIO; }
	const size_t arrays = sparse ? 3 : 1;
	uint32_t first = 0;
	if(raw.size() >= 4) memcpy(&first, raw.data(), 4);
	if(raw.size() != 4 + arrays * 4 * (size_t) DB_size || first != DB_size) {
		kmahip_set_error(KMAHIP_WRONG_DB " (%s.length.b: %zu bytes, %u templates; .comp.b: %u)", base.c_str(), raw.size(), first ? first - 1 : 0, DB_size - 1);
		return KMAHIP_EFORMAT;
	}
	o.lens.resize(DB_size);
	memcpy(o.lens.data(), raw.data() + 4, 4 * (size_t) DB_size);
	if(sparse) {
		o.slen.resize(DB_size); o.ulen.resize(DB_size);
		memcpy(o.slen.data(), raw.data() + 4 + 4 * (size_t) DB_size, 4 * (size_t) DB_size);
		memcpy(o.ulen.data(), raw.data() + 4 + 8 * (size_t) DB_size, 4 * (size_t) DB_size);
	}
	if(!all) return KMAHIP_OK;
	if(!append_slurp(base + ".name", o.names)) { kmahip_set_error("cannot read %s.name", base.c_str()); return KMAHIP_EIO; }
	if(!append_slurp(base + ".seq.b", o.seq)) { kmahip_set_error("cannot read %s.seq.b", base.c_str()); return KMAHIP_EIO; }
	size_t lines = 0, words = 0;
	for(uint8_t c : o.names) lines += c == '\n';
	for(uint32_t t = 1; t < DB_size; ++t) words += ((size_t) o.lens[t] >> 5) + 1;
	if(lines != DB_size - 1 || (!o.names.empty() && o.names.back() != '\n') || o.seq.size() != 8 * words) {
		kmahip_set_error(KMAHIP_WRONG_DB " (%s: %zu names, %zu bytes of .seq.b; %u templates of %zu words)", base.c_str(), lines, o.seq.size(), DB_size - 1, words);
		return KMAHIP_EFORMAT;
	}
	size_t w = 0;
	for(uint32_t t = 1; t < DB_size; ++t) {
		const uint32_t len = o.lens[t], rest = len & 31;
		uint64_t last;
		uint8_t *p = o.seq.data() + 8 * (w + (len >> 5));
		memcpy(&last, p, 8);
		last = rest ? last & ~(~0ull >> (2 * rest)) : 0;
		memcpy(p, &last, 8);
		w += ((size_t) len >> 5) + 1;
	}
	return KMAHIP_OK;
}

// .length.b of an appended index from whole arrays (makeindex.c:262-273): DB_size, lengths, and for a sparse index slengths, ulengths
inline int append_write_length_b(const std::string &path, uint32_t DB_size, const std::vector<uint32_t> &lens, const std::vector<uint32_t> *slen,
                                 const std::vector<uint32_t> *ulen) {
	FILE *f = fopen(path.c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s", path.c_str()); return KMAHIP_EIO; }
	bool ok = fwrite(&DB_size, 4, 1, f) == 1 && fwrite(lens.data(), 4, DB_size, f) == DB_size;
	if(slen) ok = ok && fwrite(slen->data(), 4, DB_size, f) == DB_size && fwrite(ulen->data(), 4, DB_size, f) == DB_size;
	ok = (fclose(f) == 0) && ok;
	if(!ok) { kmahip_set_error("writing %s failed", path.c_str()); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

// the files of an append are written under <prefix>.appending<ext> and take their names at the end, all of them or none
inline int append_commit(const std::string &tmp, const std::string &out, const std::vector<const char *> &exts, bool keep) {
	int rc = KMAHIP_OK;
	for(const char *e : exts) {
		if(keep && !rc && rename((tmp + e).c_str(), (out + e).c_str())) { kmahip_set_error("cannot rename %s%s to %s%s", tmp.c_str(), e, out.c_str(), e); rc = KMAHIP_EIO; }
		if(!keep || rc) remove((tmp + e).c_str());
	}
	return rc;
}

}  // namespace
