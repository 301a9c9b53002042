/* kmahip_trim.c -- `kma trim -i reads.fq[.gz] ... -o out [-qc]` on MI355X without the reference: plain C99 over the C-ABI of libkmahip.so.
 * Writes the trimmed reads back out as FASTQ -- single records to out.fq, couples (-ipe, -int) to out_int.fq, both in stream order -- and
 * with -qc the QC report out.json, byte for byte what KMA 1.5.1's `kma trim` writes (trim_main, trim.c:149-472).
 *
 *     kmahip_trim -i reads.fq.gz -o out -qc
 *     kmahip_trim -ipe r1.fq r2.fq -o out -eq 20 -ml 50
 *     kmahip_trim -i reads.fq -ipe r1.fq r2.fq -int both.fq -o out -qc -s1dev
 *
 * The command line is the reference's (trim.c:212-361), with its messages and exit statuses. -s1dev, like kmahip_map's, is our own:
 * stage 1 of the plain FASTQ files runs on the device (kmahip_ingest_dev_*: locate, trim, gate) and the text is written there too
 * (s1_fastq_kernel); .gz files, interleaved files and the records behind an odd one get the same text from the host reader.
 * Refused by name with status 2, before a file is created or a device opened: FASTA input, a run without -o (the reads on standard
 * output), `--` or no input at all (reads on standard input), several ranks, and with -qc the places where the reference's own report
 * breaks: -ml below 1 and a second -qc. */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmahip.h"

/* helpMessage (trim.c:128-147), and the one switch of our own */
static int help(FILE *out) {
	fprintf(out, "#kmahip_trim trims sequences\n");
	fprintf(out, "# %16s\t%-32s\t%s\n", "Options are:", "Desc:", "Default:");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-i", "Input file(s)", "");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-ipe", "Paired input files", "");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-int", "Interleaved input file(s)", "");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-o", "Output file prefix", "");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-qc", "Report QC", "");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-ml", "Minimum length", "16");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-xl", "Maximum length", "2147483647");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-mp", "Minimum phred", "20");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-mi", "Minimum internal phred score", "0");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-eq", "Minimum average quality", "0");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-5p", "Trim 5 prime", "0");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-3p", "Trim 3 prime", "0");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-s1dev", "Trim and write on the device", "");
	fprintf(out, "# %16s\t%-32s\t%s\n", "-h", "Shows this helpmessage", "");
	return out == stderr;
}

/* the files behind -i / -ipe / -int (trim.c:214-274): everything up to the next option; `--` (standard input) is refused by name */
static int take_files(int argc, char **argv, int *a, const char ***list, int *n) {
	while(*a + 1 < argc && (argv[*a + 1][0] != '-' || !strcmp(argv[*a + 1], "--"))) {
		if(!strcmp(argv[*a + 1], "--")) { fprintf(stderr, "kmahip_trim: -- (reads on standard input) is not built: name the files\n"); return 2; }
		const char **grown = realloc((void *) *list, (size_t) (*n + 1) * sizeof **list);
		if(!grown) { fprintf(stderr, "kmahip_trim: out of memory\n"); return 1; }
		*list = grown;
		(*list)[(*n)++] = argv[++*a];
	}
	return 0;
}

/* strtoul as the reference takes its numbers (trim.c:290-352): a missing value leaves the default */
static int number(int argc, char **argv, int *a, int *v, const char *msg, int status) {
	if(*a + 1 >= argc) { ++*a; return 0; }
	char *end;
	*v = (int) strtoul(argv[++*a], &end, 10);
	if(*end != 0) { fputs(msg, stderr); return status; }
	return 0;
}

int main(int argc, char **argv) {
	const char **se = NULL, **pe = NULL, **il = NULL, *out = NULL;
	int n_se = 0, n_pe = 0, n_il = 0, qc_opt = 0, clip5 = 0, clip3 = 0, s1dev = 0, st;
	kmahip_trim trim;
	kmahip_trim_default(&trim);
	for(int a = 1; a < argc; ++a) {
		const char *o = argv[a];
		if(!strcmp(o, "-i")) {
			const int before = n_se;
			if((st = take_files(argc, argv, &a, &se, &n_se))) return st;
			if(n_se == 0 && before == 0) { fprintf(stderr, "No files were specified.\n"); return 1; }
		} else if(!strcmp(o, "-ipe")) {
			if((st = take_files(argc, argv, &a, &pe, &n_pe))) return st;
			if(n_pe % 2) { fprintf(stderr, "Uneven number of paired end files.\n"); return 1; }
			if(n_pe == 0) { fprintf(stderr, "No paired end files were specified.\n"); return 1; }
		} else if(!strcmp(o, "-int")) {
			if((st = take_files(argc, argv, &a, &il, &n_il))) return st;
			if(n_il == 0) { fprintf(stderr, "No interleaved files were specified.\n"); return 1; }
		} else if(!strcmp(o, "-o")) { if(++a < argc) out = argv[a]; }
		else if(!strcmp(o, "-qc")) ++qc_opt;
		else if(!strcmp(o, "-ml")) { if((st = number(argc, argv, &a, &trim.min_len, "# Invalid minimum length parsed\n", 1))) return st; }
		else if(!strcmp(o, "-xl")) { if((st = number(argc, argv, &a, &trim.max_len, "# Invalid minimum length parsed\n", 1))) return st; }
		else if(!strcmp(o, "-mp")) { if((st = number(argc, argv, &a, &trim.min_phred, "# Invalid minimum phred score parsed\n", 1))) return st; }
		else if(!strcmp(o, "-mi")) { if((st = number(argc, argv, &a, &trim.hardmask_q, "# Invalid internal minimum phred score parsed\n", 1))) return st; }
		else if(!strcmp(o, "-eq")) { if((st = number(argc, argv, &a, &trim.min_q, "# Invalid average quality score parsed\n", 1))) return st; }
		else if(!strcmp(o, "-5p")) { if((st = number(argc, argv, &a, &clip5, "Invalid argument at \"-5p\".\n", 1))) return st; }
		else if(!strcmp(o, "-3p")) { if((st = number(argc, argv, &a, &clip3, "Invalid argument at \"-3p\".\n", 4))) return st; }
		else if(!strcmp(o, "-s1dev")) s1dev = 1;
		else if(!strcmp(o, "-h")) return help(stdout);
		else {
			fprintf(stderr, " Invalid option:\t%s\n", o);
			fprintf(stderr, " Printing help message:\n");
			return help(stderr);
		}
	}
	/* what is not built, by name, before anything is opened or created */
	const char *why = NULL;
	if(!(n_se + n_pe + n_il)) why = "a run without input files (the reference then reads standard input)";
	else if(!out) why = "a run without -o (the trimmed reads on standard output)";
	else if(getenv("KMAHIP_RANK") || getenv("RANK")) why = "several ranks (KMAHIP_RANK / RANK: the files are written by one process)";
	else if(qc_opt > 1) why = "a second -qc (the verbose form: the reference prints it from memory it never cleared)";
	else if(qc_opt && trim.min_len < 1) why = "-qc with -ml below 1 (the reference divides by the length of a kept read)";
	if(why) { fprintf(stderr, "kmahip_trim: not built for %s\n", why); return 2; }
	for(int k = 0; k < 3; ++k) {          /* (a look at every input's first bytes, by the host reader) */
		const char **list = k == 0 ? se : (k == 1 ? pe : il);
		const int n = k == 0 ? n_se : (k == 1 ? n_pe : n_il);
		for(int f = 0; f < n; ++f) {
			kmahip_ingest *probe = NULL;
			if(kmahip_ingest_open(list[f], NULL, &trim, &probe)) continue;          /* (a file that cannot be read is named by the run itself) */
			const int rc = kmahip_ingest_set_text(probe, 1);
			kmahip_ingest_close(probe);
			if(rc == KMAHIP_EFORMAT) { fprintf(stderr, "kmahip_trim: not built for FASTA input (%s): the trimmed reads are FASTQ records\n", list[f]); return 2; }
		}
	}
	kmahip_qc *qc = NULL;
	if(qc_opt && kmahip_qc_open(&qc)) { fprintf(stderr, "kmahip_trim: %s\n", kmahip_last_error()); return 1; }
	if(s1dev && kmahip_init(0)) { fprintf(stderr, "kmahip_trim: %s\n", kmahip_last_error()); return 1; }
	int64_t fragments = 0;
	if(kmahip_trim_files(se, n_se, pe, n_pe, il, n_il, &trim, qc, s1dev, out, &fragments)) { fprintf(stderr, "kmahip_trim: %s\n", kmahip_last_error()); return 1; }
	if(qc) {	/* trim.c:452-455 */
		char *json = malloc(strlen(out) + 8);
		if(!json) return 1;
		sprintf(json, "%s.json", out);
		if(kmahip_qc_write(qc, &trim, clip5, clip3, json)) { fprintf(stderr, "kmahip_trim: %s\n", kmahip_last_error()); return 1; }
		free(json);
		kmahip_qc_close(qc);
	}
	fprintf(stderr, "#\n# Total number of query fragment after trimming:\t%lu\n", (unsigned long) fragments);
	return 0;
}
