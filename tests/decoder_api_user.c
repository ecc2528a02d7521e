/*
 *  decoder_api_user.c -- a caller of the decoder half of fiasco.h that links against -lfiasco_amd alone: it takes the
 *  address of every name of that half (include/libfiasco_amd_decoder.h), so the link fails where one is missing, and walks
 *  the objects the way an application does, through the method pointers.  Built and run by tests/test_decoder_api.py.
 *
 *    decoder_api_user a.fco    prints "<width> <height> <length> <rate> <color>" of the stream; no device needed
 */
#include <stdio.h>
#include "libfiasco_amd_decoder.h"

static const void *const names[] = {
    (const void *) fiasco_d_options_new, (const void *) fiasco_d_options_delete, (const void *) fiasco_d_options_set_smoothing,
    (const void *) fiasco_d_options_set_magnification, (const void *) fiasco_d_options_set_4_2_0_format,
    (const void *) fiasco_decoder_new, (const void *) fiasco_decoder_delete, (const void *) fiasco_decoder_write_frame,
    (const void *) fiasco_decoder_get_frame, (const void *) fiasco_decoder_get_width, (const void *) fiasco_decoder_get_height,
    (const void *) fiasco_decoder_is_color, (const void *) fiasco_decoder_get_rate, (const void *) fiasco_decoder_get_length,
    (const void *) fiasco_decoder_get_title, (const void *) fiasco_decoder_get_comment,
    (const void *) fiasco_image_new, (const void *) fiasco_image_delete, (const void *) fiasco_image_get_width,
    (const void *) fiasco_image_get_height, (const void *) fiasco_image_is_color,
    (const void *) fiasco_renderer_new, (const void *) fiasco_renderer_delete, (const void *) fiasco_renderer_render,
    (const void *) fiasco_get_error_message,
};

int main(int argc, char **argv)
{
    fiasco_d_options_t *o = fiasco_d_options_new();
    fiasco_renderer_t *r = fiasco_renderer_new(0xf800, 0x07e0, 0x001f, 16, 0);
    fiasco_decoder_t *d;
    unsigned i;
    for (i = 0; i < sizeof names / sizeof *names; i++) if (!names[i]) return 3;
    if (argc != 2 || !o || !r) return 2;
    if (!o->delete_ || !o->set_smoothing || !o->set_magnification || !o->set_4_2_0_format || !r->render || !r->delete_) return 4;
    if (!o->set_smoothing(o, 35) || !o->set_magnification(o, 0) || !o->set_4_2_0_format(o, 0)) return 5;
    d = fiasco_decoder_new(argv[1], o);
    if (!d) { fprintf(stderr, "%s\n", fiasco_get_error_message()); return 1; }
    if (!d->delete_ || !d->write_frame || !d->get_frame || !d->get_length || !d->get_rate || !d->get_width || !d->get_height || !d->get_title
        || !d->get_comment || !d->is_color) return 4;
    printf("%u %u %u %u %d\n", d->get_width(d), d->get_height(d), d->get_length(d), d->get_rate(d), d->is_color(d));
    d->delete_(d);
    r->delete_(r);
    o->delete_(o);
    return 0;
}
