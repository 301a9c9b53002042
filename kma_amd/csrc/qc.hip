// qc.hip -- the QC report of `kma ... -qc` / `kma trim -qc` (kmahip.h: kmahip_qc_*) and `kma trim` over files (kmahip_trim_files).
// Behaviour restated from init_QCstat / rescale_ldist / update_QCstat / print_QCstat (qc.c:24-65, 85-104, 167-262) and trim_main
// (trim.c:363-471). Host-only translation unit: the readers (ingest.hip, ingest_dev.hip) feed the accumulator, in stream order.
//
// Two of its quantities depend on floating-point order and are therefore made here and nowhere else: Eeq, the sum of the counted
// sequences' sp in stream order, and the quality bin (int) ceil(-10 * log10(sp / len)), whose argument sits within an ulp of a whole
// number for a read of uniform quality -- the bin is whatever this host's log10 says, as it is for the reference on the same host.
#include "kmahip_internal.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct kmahip_qc {
	kmahip_qc_stats s;
};

namespace {

// rescale_ldist (qc.c:50-65): the bins folded from resolution `from` to `to`; bin 0 stays where it is
void fold(uint32_t *ldist, int from, int to) {
	const int mask = to - from;
	if(mask <= 0) return;
	for(int i = 1; i < 512; ++i) { const uint32_t v = ldist[i]; ldist[i] = 0; ldist[i >> mask] += v; }
}

// update_QCstat's `if(src->maxlen < len)` branch (qc.c:92-101) without the verbose form
void raise_maxlen(kmahip_qc_stats &s, int len) {
	if(s.maxlen >= len) return;
	if(512 <= (len >> s.qresolution)) {
		int res = s.qresolution;
		while(512 <= (len >> ++res));
		fold(s.ldist, s.qresolution, res);
		s.qresolution = res;
	}
	s.maxlen = len;
}

inline int qbin(double sp, int len) { return (int) ceil(-10 * log10(sp / len)); }

}  // namespace

extern "C" int kmahip_qc_open(kmahip_qc **out) {
	if(!out) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	*out = new kmahip_qc();
	memset(&(*out)->s, 0, sizeof (*out)->s);
	return KMAHIP_OK;
}

extern "C" void kmahip_qc_close(kmahip_qc *qc) { delete qc; }

extern "C" int kmahip_qc_get(const kmahip_qc *qc, kmahip_qc_stats *out) {
	if(!qc || !out) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	*out = qc->s;
	return KMAHIP_OK;
}

void kmahip_qc_add_seq(kmahip_qc *qc, int len, int gc, int ns, double sp) {
	kmahip_qc_stats &s = qc->s;
	s.count++; s.bpcount += (uint64_t) len; s.totgc += (uint64_t) gc; s.totns += (uint64_t) ns;
	s.Eeq += sp;
	raise_maxlen(s, len);
	s.qdist[qbin(sp, len) & 255]++;
	s.ldist[len >> s.qresolution]++;
}

void kmahip_qc_add_pass(kmahip_qc *qc, uint64_t count, uint64_t bp, uint64_t gc, uint64_t ns, int maxlen, const uint32_t *hist, int res,
                        const KmaQcPair *pairs, size_t n_pairs) {
	kmahip_qc_stats &s = qc->s;
	s.count += count; s.bpcount += bp; s.totgc += gc; s.totns += ns;
	raise_maxlen(s, maxlen);
	// the pass's bins are at least as coarse as its own longest read needs: both sides meet at the coarser resolution (folding is
	// binning at the final resolution, so neither the order of the reads nor that of the passes matters)
	if(count) {
		if(res > s.qresolution) { fold(s.ldist, s.qresolution, res); s.qresolution = res; }
		const int mask = s.qresolution - res;
		for(int i = 0; i < 512; ++i) if(hist[i]) s.ldist[i >> mask] += hist[i];
	}
	for(size_t i = 0; i < n_pairs; ++i) {
		s.Eeq += pairs[i].sp;
		s.qdist[qbin(pairs[i].sp, pairs[i].len) & 255]++;
	}
}

void kmahip_qc_add_read(kmahip_qc *qc, uint64_t org_count, uint64_t org_bp, uint64_t org_frag, uint64_t frag) {
	kmahip_qc_stats &s = qc->s;
	s.org_count += org_count; s.org_bpcount += org_bp; s.org_fragcount += org_frag; s.fragcount += frag;
}

void kmahip_qc_end_reader(kmahip_qc *qc, bool paired, int phred) {
	if(!paired || qc->s.Eeq) qc->s.phred_scale = phred;
}

extern "C" int kmahip_qc_write(const kmahip_qc *qc, const kmahip_trim *trim, int clip5, int clip3, const char *path) {
	if(!qc || !trim || !path) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	FILE *dest = fopen(path, "wb");
	if(!dest) { kmahip_set_error("cannot open %s", path); return KMAHIP_EIO; }
	const kmahip_qc_stats &s = qc->s;
	const int minPhred = trim->min_phred < trim->hardmask_q ? trim->hardmask_q : trim->min_phred;
	fprintf(dest, "{\n");
	fprintf(dest, "\t\"Maximum Trim length\": %d,\n", trim->max_len);
	fprintf(dest, "\t\"Minimum Trim length\": %d,\n", trim->min_len);
	fprintf(dest, "\t\"5\'-clip\": %d,\n", clip5);
	fprintf(dest, "\t\"3\'-clip\": %d,\n", clip3);
	if(s.Eeq) {
		fprintf(dest, "\t\"Minimum Q\": %d,\n", trim->min_q);
		fprintf(dest, "\t\"End Trim Q\": %d,\n", minPhred);
		fprintf(dest, "\t\"Hard Mask Q\": %d,\n", trim->hardmask_q);
		fprintf(dest, "\t\"Phred Scale\": %d,\n", s.phred_scale);
	}
	fprintf(dest, "\t\"Fragment Count\": %lu,\n", (unsigned long) s.fragcount);
	fprintf(dest, "\t\"Org. Fragment Count\": %lu,\n", (unsigned long) s.org_fragcount);
	fprintf(dest, "\t\"Sequence Count\": %lu,\n", (unsigned long) s.count);
	fprintf(dest, "\t\"Org. Sequence Count\": %lu,\n", (unsigned long) s.org_count);
	fprintf(dest, "\t\"Bp Count\": %lu,\n", (unsigned long) s.bpcount);
	fprintf(dest, "\t\"Org. Bp Count\": %lu,\n", (unsigned long) s.org_bpcount);
	fprintf(dest, "\t\"Mean Read Length\": %f,\n", s.count ? ((double) s.bpcount / s.count) : 0);
	fprintf(dest, "\t\"Org. Mean Read Length\": %f,\n", s.org_count ? ((double) s.org_bpcount / s.org_count) : 0);
	fprintf(dest, "\t\"GC Content\": %f,\n", (s.bpcount - s.totns) ? ((double) s.totgc / (s.bpcount - s.totns)) : 0);
	fprintf(dest, "\t\"Max Sequence Length\": %d,\n", s.maxlen);
	// N50 (qc.c:200-235), in the reference's own integer and floating-point types
	const uint32_t *dist = s.ldist;
	const int scale = 1 << s.qresolution;
	int n50;
	if((unsigned long) (s.maxlen << 1) < s.bpcount) {
		n50 = 0;
		double p = 0;
		unsigned long tot = 0;
		if(s.qresolution) {
			for(int i = 0; i < 511; ++i) {
				if(dist[i]) {
					p = (double) (dist[i + 1]) / (dist[i] + dist[i + 1]);
					tot += (n50 + p * scale) * dist[i];
					if(s.bpcount < (tot << 1)) { n50 += p * scale; i = 512; }
					else n50 += scale;
				} else n50 += scale;
			}
		} else {
			for(int i = 0; i < 512; ++i) {
				tot += (unsigned) i * dist[i];
				if(s.bpcount < (tot << 1)) { n50 = i; i = 512; }
			}
		}
	} else n50 = s.maxlen;
	fprintf(dest, "\t\"N50\": %d,\n", n50);
	if(s.Eeq) {
		dist = s.qdist;
		fprintf(dest, "\t\"E(Q)\": %f,\n", -10 * log10(s.Eeq / s.bpcount));
		fprintf(dest, "\t\"Q Distribution\": [%d, %d, %d, %d", (int) dist[0], (int) dist[1], (int) dist[2], (int) dist[3]);
		for(int i = 4; i < 256; i += 4) fprintf(dest, ", %d, %d, %d, %d", (int) dist[i], (int) dist[i + 1], (int) dist[i + 2], (int) dist[i + 3]);
		fprintf(dest, "],\n");
	}
	dist = s.ldist;
	fprintf(dest, "\t\"Length Resolution\": %d,\n", scale);
	fprintf(dest, "\t\"Length Distribution\": [%d, %d, %d, %d", (int) dist[0], (int) dist[1], (int) dist[2], (int) dist[3]);
	for(int i = 4; i < 512; i += 4) fprintf(dest, ", %d, %d, %d, %d", (int) dist[i], (int) dist[i + 1], (int) dist[i + 2], (int) dist[i + 3]);
	fprintf(dest, "]\n");
	fprintf(dest, "}\n");
	if(fclose(dest)) { kmahip_set_error("cannot write %s", path); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

// trim_main (trim.c:363-471) behind its options: the single-end files, the couples of mate files, the interleaved files, one reader
// after the other into the two text files
extern "C" int kmahip_trim_files(const char *const *se, int n_se, const char *const *pe, int n_pe, const char *const *il, int n_il,
                                 const kmahip_trim *trim, kmahip_qc *qc, int s1dev, const char *out_prefix, int64_t *fragments) {
	if(!out_prefix || n_se < 0 || n_pe < 0 || (n_pe & 1) || n_il < 0 || (n_se && !se) || (n_pe && !pe) || (n_il && !il)) { kmahip_set_error("bad argument"); return KMAHIP_EINVAL; }
	kmahip_trim T;
	if(trim) T = *trim; else kmahip_trim_default(&T);
	if(qc && T.min_len < 1) { kmahip_set_error("a QC report needs a minimum length of 1 at least (the reference divides by the length of a kept read)"); return KMAHIP_EINVAL; }
	const std::string base = out_prefix;
	FILE *out[2] = {fopen((base + ".fq").c_str(), "wb"), nullptr};
	if(out[0] && n_pe + n_il) out[1] = fopen((base + "_int.fq").c_str(), "wb");
	int rc = KMAHIP_OK;
	if(!out[0] || (n_pe + n_il && !out[1])) { kmahip_set_error("cannot open %s.fq / %s_int.fq", out_prefix, out_prefix); rc = KMAHIP_EIO; }
	int64_t total = 0;
	const int n_readers = n_se + n_pe / 2 + n_il;
	for(int r = 0; r < n_readers && !rc; ++r) {
		kmahip_ingest *in = nullptr;
		kmahip_ingest_dev *dev = nullptr;
		const bool interleaved = r >= n_se + n_pe / 2;
		const char *p1 = r < n_se ? se[r] : (!interleaved ? pe[2 * (r - n_se)] : il[r - n_se - n_pe / 2]);
		const char *p2 = r < n_se || interleaved ? nullptr : pe[2 * (r - n_se) + 1];
		if(s1dev && !interleaved) {
			// (a file the device reader does not cover says so before it touches the device: the host reader's then)
			rc = kmahip_ingest_dev_open(p1, p2, &T, &dev);
			if(rc == KMAHIP_EFORMAT) { rc = KMAHIP_OK; dev = nullptr; }
			if(!rc && dev) rc = kmahip_ingest_dev_set_text(dev, 1);
			if(!rc && dev && qc) rc = kmahip_ingest_dev_set_qc(dev, qc);
		}
		if(!rc && !dev) {
			rc = interleaved ? kmahip_ingest_open_interleaved(p1, &T, &in) : kmahip_ingest_open(p1, p2, &T, &in);
			if(!rc) rc = kmahip_ingest_set_text(in, 1);
			if(!rc && qc) rc = kmahip_ingest_set_qc(in, qc);
		}
		while(!rc) {
			kmahip_read_batch b;
			rc = dev ? kmahip_ingest_dev_next(dev, 1 << 20, &b) : kmahip_ingest_next(in, 1 << 20, &b);
			if(rc || b.reads.n_reads == 0) break;
			total += b.records;
			for(int k = 0; k < 2 && !rc; ++k) {
				const char *text = nullptr;
				int64_t bytes = 0;
				rc = dev ? kmahip_ingest_dev_text(dev, k, &text, &bytes) : kmahip_ingest_text(in, k, &text, &bytes);
				if(!rc && bytes && (!out[k] || fwrite(text, 1, (size_t) bytes, out[k]) != (size_t) bytes)) { kmahip_set_error("cannot write the trimmed reads"); rc = KMAHIP_EIO; }
			}
		}
		if(!rc && dev) rc = kmahip_ingest_dev_status(dev);
		if(!rc && in) rc = kmahip_ingest_status(in);
		if(dev) kmahip_ingest_dev_close(dev);
		if(in) kmahip_ingest_close(in);
	}
	for(int k = 0; k < 2; ++k) if(out[k] && fclose(out[k]) && !rc) { kmahip_set_error("cannot write the trimmed reads"); rc = KMAHIP_EIO; }
	if(fragments) *fragments = total;
	return rc;
}
