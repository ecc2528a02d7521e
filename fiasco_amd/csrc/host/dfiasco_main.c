/*
 *  dfiasco_main.c -- thin command line front end over the decoder API (include/libfiasco_amd_decoder.h), as
 *  cfiasco_main.c is for the coder: own implementation of what reference bin/dwfa.c does without a window.  Options and
 *  defaults follow bin/dwfa.c:88-105, the names of the files written bin/dwfa.c:197-277: `base.suffix' for a stream of one
 *  frame, `base.%0*d.suffix' for several, base and suffix from the output name or, without one, from the input name.
 *  --double, --panel and --framerate belong to the window: parsed and dropped.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <getopt.h>
#include "libfiasco_amd_decoder.h"

static void die(const char *prog)
{
    fprintf(stderr, "%s: %s\n", prog, fiasco_get_error_message());
    exit(1);
}

/* get_output_template (bin/dwfa.c:237-277) */
static void output_template(const char *image_name, const char *wfa_name, int color, char **base, const char **suffix)
{
    char *dot = NULL;
    if (!wfa_name || !strcmp(wfa_name, "-")) wfa_name = "stdin";
    if (!image_name || !image_name[0] || !strcmp(image_name, "-")) *base = strdup(wfa_name);
    else { *base = strdup(image_name); dot = *base ? strrchr(*base, '.') : NULL; }
    if (!*base) { fprintf(stderr, "Out of memory.\n"); exit(1); }
    *suffix = color ? "ppm" : "pgm";
    if (dot) {
        *dot = 0;
        if (dot[1]) *suffix = dot + 1;
    }
}

static void decode_file(const char *prog, const char *wfa_name, const char *image_name, fiasco_d_options_t *options)
{
    fiasco_decoder_t *d = fiasco_decoder_new(wfa_name, options);
    unsigned frames, n;
    int digits;
    char *base, *filename;
    const char *suffix;
    if (!d) die(prog);
    if (!fiasco_decoder_get_width(d) || !fiasco_decoder_get_height(d) || !(frames = fiasco_decoder_get_length(d))) die(prog);
    output_template(image_name, wfa_name, fiasco_decoder_is_color(d), &base, &suffix);
    digits = frames > 1 ? (int) (log10((double) (frames - 1)) + 1) : 1;
    filename = (char *) malloc(strlen(base) + strlen(suffix) + 32);
    if (!filename) { fprintf(stderr, "Out of memory.\n"); exit(1); }
    for (n = 0; n < frames; n++) {
        if (frames == 1) {
            if (!strcmp(image_name, "-")) strcpy(filename, "-");
            else sprintf(filename, "%s.%s", base, suffix);
        } else {
            fprintf(stderr, "Decoding frame %d to file `%s.%0*d.%s\n", (int) n, base, digits, (int) n, suffix);
            sprintf(filename, "%s.%0*d.%s", base, digits, (int) n, suffix);
        }
        if (!fiasco_decoder_write_frame(d, filename)) die(prog);
    }
    free(filename); free(base);
    fiasco_decoder_delete(d);
}

int main(int argc, char **argv)
{
    static struct option lo[] = {
        {"output", 1, 0, 'o'}, {"double", 0, 0, 'd'}, {"fast", 0, 0, 'r'}, {"panel", 0, 0, 'p'},
        {"magnify", 1, 0, 'm'}, {"framerate", 1, 0, 'F'}, {"smoothing", 1, 0, 's'}, {0, 0, 0, 0}
    };
    const char *image_name = "-";
    int smoothing = -1, magnify = 0, fast = 0, ch;
    fiasco_d_options_t *options;

    while ((ch = getopt_long(argc, argv, "o:drpm:F:s:", lo, NULL)) != -1)
        switch (ch) {
        case 'o': image_name = optarg; break;
        case 'm': magnify = atoi(optarg); break;
        case 's': smoothing = atoi(optarg); break;
        case 'r': fast = 1; break;
        case 'd': case 'p': case 'F': break;            /* the window's */
        default:
            fprintf(stderr, "usage: %s [-o FILE] [-m NUM] [-s NUM] [-r] [FIASCO-FILE]...\n", argv[0]);
            return 2;
        }
    options = fiasco_d_options_new();
    if (!options) die(argv[0]);
    if (!fiasco_d_options_set_smoothing(options, smoothing < -1 ? -1 : smoothing)) die(argv[0]);
    if (!fiasco_d_options_set_magnification(options, magnify)) die(argv[0]);
    if (!fiasco_d_options_set_4_2_0_format(options, fast)) die(argv[0]);
    if (optind >= argc) decode_file(argv[0], "-", image_name, options);
    else for (; optind < argc; optind++) decode_file(argv[0], argv[optind], image_name, options);
    fiasco_d_options_delete(options);
    return 0;
}
