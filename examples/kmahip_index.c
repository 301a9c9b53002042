/* kmahip_index.c -- `kma index -i templates.fsa [more.fsa ...] (or -batch list.txt) -o prefix [-k k] [-deCon host.fsa ...]` on an MI355X:
 * plain C99 over kmahip_index_build / kmahip_index_build_decon / kmahip_index_build_sparse (the k-mers are sorted and made unique on
 * the device). Writes prefix.comp.b / .length.b / .seq.b / .name, which the reference and libkmahip load alike, and with -deCon
 * prefix.decon.comp.b beside them (what `kma ... -deCon` and `kmahip_map ... -deCon` map against). With -Sparse the index is the
 * sparse one (`kma -Sparse`, `kmahip_map -Sparse`): only the k-mers behind the prefix, of both strands; -ML is its length gate.
 *
 *     kmahip_index -i genes.fsa -o genes [-k 16] [-deCon host.fsa phix.fsa]
 *     kmahip_index -i genes.fsa -o genes_sparse -Sparse TG [-ML 100]
 *     kmahip_index -i genes.fsa -o genes_thin -Sparse TG -hq 0.9 -ht 0.9 -and > clusters.tsv
 *     kmahip_index -t_db genes -i new.fsa [-o genes_2] [-deCon host.fsa]
 *     kmahip_index -t_db genes -deCon host.fsa
 *
 * -t_db <prefix> (index.c:221-229, 529-557, 616-732): templates are appended to the index that exists, over kmahip_index_append. k and
 * the sparse prefix are the index's: -k and -Sparse beside -t_db are taken and overridden, as in the reference. Without -o the append
 * happens in place; without -i, -deCon writes <prefix>.decon.comp.b for the index as it is. -hq / -ht / -ML are not built with it.
 * -hq / -ht / -and (index.c:309-350, qualcheck.c:81-324): homology reduction of a sparse index over kmahip_index_build_sparse_hom; a
 * template too similar to those kept before it gets no id, and every template that reaches the gates gets a cluster line on standard
 * output. Without -Sparse the three options are taken without effect, as in the reference (updateDBs never calls QualCheck).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmahip.h"

#define USAGE "usage: kmahip_index (-i <fasta> [<fasta> ...] | -batch <file of paths>) -o <index prefix> [-k <k-mer length, 4 ... 16>] " \
              "[-t_db <index to append to> (then -o is optional: in place; -i is optional beside -deCon)] " \
              "[-deCon <fasta> [<fasta> ...]] [-Sparse [<prefix>|-] [-ML <minimum length>] [-hq <query homology, 0 ... 1>] [-ht <template homology, 0 ... 1>] [-and]]\n"

/* index.c:451-474: the letters the reference's table maps to 0 ... 3; anything else, or nothing at all, is no prefix */
static int valid_prefix(const char *s) {
	if(!strcmp(s, "-")) return 1;
	if(!*s) return 0;
	for(; *s; ++s) if(!strchr("ARMDarmdCYBcybGSKVgskvTWHUtwhu", *s)) return 0;
	return 1;
}

int main(int argc, char **argv) {
	const char *inputs[256], *decon[256], *out = NULL, *sparse = NULL, *t_db = NULL;
	int n_in = 0, n_decon = 0, decon_opt = 0, k = 16, ml_opt = 0;
	long min_len = 0;
	double hom_q = 1.0, hom_t = 1.0;
	int and_mode = 0, hom_opt = 0;
	for(int a = 1; a < argc; ++a) {
		if(!strcmp(argv[a], "-i")) { while(a + 1 < argc && argv[a + 1][0] != '-' && n_in < 256) inputs[n_in++] = argv[++a]; }
		else if(!strcmp(argv[a], "-batch") && a + 1 < argc) {          /* index.c:351-401: a file that lists the inputs, one path a line */
			FILE *f = fopen(argv[++a], "rb");
			static char lines[256][4096];
			if(!f) { fprintf(stderr, "kmahip_index: cannot open %s\n", argv[a]); return 1; }
			while(n_in < 256 && fgets(lines[n_in], sizeof lines[0], f)) {
				size_t l = strlen(lines[n_in]);
				while(l && (lines[n_in][l - 1] == '\n' || lines[n_in][l - 1] == '\r' || lines[n_in][l - 1] == ' ' || lines[n_in][l - 1] == '\t')) lines[n_in][--l] = 0;
				if(l) { inputs[n_in] = lines[n_in]; ++n_in; }
			}
			fclose(f);
		}
		else if(!strcmp(argv[a], "-deCon")) {          /* index.c:200-220: every argument up to the next option; `--` is standard input there */
			decon_opt = 1;
			while(a + 1 < argc && (argv[a + 1][0] != '-' || !strcmp(argv[a + 1], "--")) && n_decon < 256) {
				if(!strcmp(argv[a + 1], "--")) { fprintf(stderr, "kmahip_index: -deCon -- (contamination from standard input) is not built: give a file\n"); return 2; }
				decon[n_decon++] = argv[++a];
			}
			if(n_decon == 0) { fprintf(stderr, "No deCon file specified.\n"); return 1; }
		}
		else if(!strcmp(argv[a], "-o") && a + 1 < argc) out = argv[++a];
		else if(!strcmp(argv[a], "-t_db") && a + 1 < argc) t_db = argv[++a];          /* index.c:221-229 */
		else if(!strcmp(argv[a], "-k") && a + 1 < argc) k = atoi(argv[++a]);
		else if(!strcmp(argv[a], "-Sparse")) {         /* index.c:451-474: the next argument whatever it is; none, or "-": no prefix */
			sparse = a + 1 < argc ? argv[++a] : "-";
			if(!valid_prefix(sparse)) { fprintf(stderr, "Invalid prefix.\n"); return 1; }
		}
		else if(!strcmp(argv[a], "-ML") && a + 1 < argc) {          /* index.c:315-326 */
			char *end;
			min_len = strtol(argv[++a], &end, 10);
			ml_opt = 1;
			if(*end) { fprintf(stderr, "# Invalid minimum length parsed\n"); return 1; }
			if(min_len <= 0) { fprintf(stderr, "# Invalid minimum length parsed, using default\n"); min_len = 0; }
			if(min_len > 0x7FFFFFFF) min_len = 0x7FFFFFFF;
		}
		else if(!strcmp(argv[a], "-and")) and_mode = 1;          /* index.c:309 */
		else if(!strcmp(argv[a], "-hq") || !strcmp(argv[a], "-ht")) {          /* index.c:327-350: no value behind it: nothing happens */
			double *dst = argv[a][2] == 'q' ? &hom_q : &hom_t;
			hom_opt = 1;
			if(a + 1 < argc) {
				char *end;
				*dst = strtod(argv[a + 1], &end);
				if(*end) { fprintf(stderr, "Invalid argument at \"%s\".\n", argv[a]); return 1; }
				if(*dst < 0) { fprintf(stderr, "Invalid -hq\n"); *dst = 1.0; }          /* (these words for both options) */
				++a;
			}
		}
		else { fprintf(stderr, USAGE); return 2; }
	}
	/* what is not built is refused by name, before a file or the device is opened */
	if(t_db && hom_opt) { fprintf(stderr, "kmahip_index: -hq / -ht are not built with -t_db (the homology check against the templates already in the index)\n"); return 2; }
	if(t_db && ml_opt) { fprintf(stderr, "kmahip_index: -ML is not built with -t_db\n"); return 2; }
	if(t_db) {
		/* index.c:494-500: what must be there; k and the prefix are the index's, whatever -k and -Sparse said (index.c:535-546) */
		if(!n_in && !n_decon) { fprintf(stderr, "No inputfiles defined.\n"); return 255; }
		if(kmahip_init(0) || kmahip_index_append(t_db, inputs, n_in, decon, n_decon, out)) { fprintf(stderr, "kmahip_index: %s\n", kmahip_last_error()); return 1; }
		return 0;
	}
	if(sparse && decon_opt) { fprintf(stderr, "kmahip_index: -Sparse is not built for -deCon (deConNode_sparse)\n"); return 2; }
	if(ml_opt && !sparse) { fprintf(stderr, "kmahip_index: -ML is not built for a build without -Sparse\n"); return 2; }
	if(sparse && ml_opt && min_len > 0 && hom_t < 1) {
		fprintf(stderr, "kmahip_index: -ht is not built with -ML (templateCheck leaves its scores uncleared behind a template below -ML, qualcheck.c:287)\n");
		return 2;
	}
	if(!n_in && n_decon) { fprintf(stderr, "Nothing to update.\n"); return 0; }          /* index.c:498-500 */
	if(!n_in || !out) { fprintf(stderr, "kmahip_index: -i and -o are required\n"); return 2; }
	if(kmahip_init(0) || (sparse ? kmahip_index_build_sparse_hom(inputs, n_in, out, k, k, sparse, (int) min_len, hom_q, hom_t, and_mode, "-")
	                      : decon_opt ? kmahip_index_build_decon(inputs, n_in, decon, n_decon, out, k) : kmahip_index_build(inputs, n_in, out, k))) {
		fprintf(stderr, "kmahip_index: %s\n", kmahip_last_error()); return 1;
	}
	return 0;
}
