/* kmahip_dist.c -- `kma dist -t_db prefix [-o file] [-d methods] [-f format]` on an MI355X: plain C99 over kmahip_tdist_open /
 * _count / _write. Reads prefix.comp.b and prefix.name (any form of index the reference writes), counts for every pair of templates
 * the k-mers they share and writes the PHYLIP matrices of the chosen measures, byte for byte the reference's file. What the program
 * prints for -dh, -fh, -h and for a command line it cannot take, and the status it ends with, are the reference's: the texts below
 * are held to the recorded ones by tests/test_tdist_cli.py. -m, -tmp dir and -t n are taken without effect (the matrix lives in
 * device memory, and the device is the threads).
 *
 *     kmahip_dist -t_db genes [-o genes.phy] [-d 1] [-f 1]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmahip.h"

static const char METHODS_TEXT[] =
	"# Distance / Similarity calculation methods, add them to combine them:\n"
	"#\n"
	"#        1\tk-mer hamming distance\n"
	"#        2\tShared k-mers\n"
	"#        4\tk-mer query coverage\n"
	"#        8\tk-mer template coverage\n"
	"#       16\tk-mer avg. coverage\n"
	"#       32\tk-mer inv. avg. coverage\n"
	"#       64\tJaccard distance\n"
	"#      128\tJaccard similarity\n"
	"#      256\tCosine distance\n"
	"#      512\tCosine similarity\n"
	"#     1024\tSzymkiewicz\xe2\x80\x93Simpson similarity\n"
	"#     2048\tSzymkiewicz\xe2\x80\x93Simpson dissimilarity\n"
	"#     4096\tChi-square distance\n"
	"#\n";

static const char FORMATS_TEXT[] =
	"# Format flags output, add them to combine them.\n"
	"#\n"
	"#        1\tRelaxed Phylip\n"
	"#        4\tInclude distance method(s) in phylip file\n";

static const char OPTIONS_TEXT[] =
	"#kma dist calculates distances between templates from a kma index\n"
	"#     Options are:\tDesc:                           \tDefault:\n"
	"#            -t_db\tTemplate DB                     \t\n"
	"#               -o\tOutput file                     \tDB\n"
	"#               -f\tOutput flags                    \t1\n"
	"#              -fh\tHelp on option \"-f\"             \t\n"
	"#               -d\tDistance method                 \t1\n"
	"#              -dh\tHelp on option \"-d\"             \t\n"
	"#               -m\tAllocate matrix on the disk     \tFalse\n"
	"#             -tmp\tSet directory for temporary files\t\n"
	"#               -t\tNumber of threads               \t1\n"
	"#               -h\tShows this helpmessage          \t\n";

/* what an option is followed by */
enum { NOTHING, A_PATH, A_NUMBER, A_DIRECTORY, A_TEXT };

static const struct option {
	const char *name;
	int wants;
	const char *text;         /* A_TEXT: printed, and the program ends with status 0 */
	const char *missing;      /* the option the `Missing argument` line names (for -t_db the reference names -o) */
} OPTIONS[] = {
	{"-t_db", A_PATH, NULL, "-o"},   {"-o", A_PATH, NULL, "-o"},         {"-f", A_NUMBER, NULL, "-f"}, {"-d", A_NUMBER, NULL, "-d"},
	{"-t", A_NUMBER, NULL, "-t"},    {"-tmp", A_DIRECTORY, NULL, NULL},  {"-m", NOTHING, NULL, NULL},  {"-fh", A_TEXT, FORMATS_TEXT, NULL},
	{"-dh", A_TEXT, METHODS_TEXT, NULL}, {"-h", A_TEXT, OPTIONS_TEXT, NULL},
};

static int fail(const char *line, const char *option) {
	fprintf(stderr, line, option);
	return 1;
}

int main(int argc, char **argv) {
	const char *db = NULL, *out = NULL;
	char *default_out = NULL;
	long numbers[3] = {1, 1, 1};          /* -f, -d, -t */
	kmahip_tdist *td = NULL;
	int rc;

	/* the options in the order they stand: the first help option, or the first mistake, ends the program */
	for(int a = 1; a < argc; ++a) {
		const struct option *o = NULL;
		const char *value = a + 1 < argc ? argv[a + 1] : NULL;
		for(size_t i = 0; i < sizeof OPTIONS / sizeof OPTIONS[0]; ++i) if(!strcmp(argv[a], OPTIONS[i].name)) o = &OPTIONS[i];
		if(!o) {
			fprintf(stderr, argv[a][0] == '-' ? "Unknown option:%s\n" : "Unknown argument:%s\n", argv[a]);
			fputs(OPTIONS_TEXT, stderr);
			return 1;
		}
		if(o->wants == A_TEXT) { fputs(o->text, stdout); return 0; }
		if(o->wants == NOTHING) continue;
		if(!value) {
			if(o->wants == A_DIRECTORY) continue;          /* (a last -tmp without a directory passes) */
			return fail("Missing argument at \"%s\".\n", o->missing);
		}
		++a;
		if(o->wants == A_PATH) { if(o->name[1] == 'o') out = value; else db = value; }
		else if(o->wants == A_DIRECTORY) { if(value[0] == '-') return fail("Invalid value parsed at \"%s\".\n", o->name); }
		else {
			char *end;
			const long v = (long) strtoul(value, &end, 10);
			if(*end) return fail("Invalid value parsed at \"%s\".\n", o->name);
			numbers[o->name[1] == 'f' ? 0 : o->name[1] == 'd' ? 1 : 2] = v;
		}
	}
	if(!db) return fail("%s", "Too few arguments handed.\n");
	if(!out) {
		default_out = malloc(strlen(db) + 8);
		if(!default_out) return fail("%s", "kmahip_dist: out of memory\n");
		sprintf(default_out, "%s.phy", db);
		out = default_out;
	}

	if(kmahip_init(0)) { fprintf(stderr, "kmahip_dist: %s\n", kmahip_last_error()); free(default_out); return 1; }
	rc = kmahip_tdist_open(db, &td);
	if(rc == KMAHIP_EFORMAT) fprintf(stderr, "Wrong format of DB.\n");          /* (the reference's line for a file it cannot read) */
	if(!rc) rc = kmahip_tdist_count(td);
	if(!rc) rc = kmahip_tdist_write(td, out, (int) numbers[1], (int) numbers[0]);
	if(rc) fprintf(stderr, "kmahip_dist: %s\n", kmahip_last_error());
	kmahip_tdist_close(td);
	free(default_out);
	return rc ? 1 : 0;
}
