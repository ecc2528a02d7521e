/*
 *  fa_decoder.c -- the decoder half of fiasco.h (include/libfiasco_amd_decoder.h): the options, the decoder, the image and
 *  the renderer objects, restated after codec/options.c:716-875, codec/dfiasco.c, lib/image.c and lib/dither.c.
 *
 *  The objects are host C; the frames are the device's.  A decoder owns one stream that was read (fa_stream.c) and one
 *  cursor over it (fa_cursor): a call for the next display frame advances the cursor, whose flights hand the shown planes
 *  of every wanted frame to fa_dev_outlet_run (csrc/hip/decoder_outlet.inc) in device buffers.  The decoder keeps the
 *  buffers of frames decoded ahead (ready[]) until their turn; an image takes its buffer over and, when it is deleted,
 *  gives it back to the decoder for a frame to come (d_pool) or, after the decoder went, frees it.  For its lifetime the
 *  decoder also keeps what its share of the device needs per call -- the HIP stream, the events and the arena of its flights
 *  (fa_outlet.keep) -- and the staging memory of write_frame.  Rendering and the PNM writer launch the existing kernels on those planes
 *  (fiasco_amd_planes_render_device[_420], fiasco_amd_planes_to_pixels_device) into staging memory the renderer / the
 *  decoder keeps, and copy the result to the host once.
 */
#include <errno.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fa_host.h"
#include "libfiasco_amd_stream.h"
#include "libfiasco_amd_decoder.h"

/* ---------------------------------------------------------------- options (codec/options.c:716-875) */

typedef struct d_options { char id[9]; int smoothing, magnification, format_420; } d_options;

static d_options *cast_d_options(const fiasco_d_options_t *options)
{
    d_options *o = options ? (d_options *) options->private_ : NULL;
    if (!o) { fa_set_error("Parameter `%s' not defined (NULL).", "options"); return NULL; }
    if (strcmp(o->id, "DOFIASCO")) { fa_set_error("Parameter `options' doesn't match required type."); return NULL; }
    return o;
}

fiasco_d_options_t *fiasco_d_options_new(void)
{
    d_options *o = (d_options *) fiasco_calloc(1, sizeof *o);
    fiasco_d_options_t *pub = (fiasco_d_options_t *) fiasco_calloc(1, sizeof *pub);
    if (!o || !pub) { free(o); free(pub); fa_set_error("Out of memory."); return NULL; }
    pub->private_ = o;
    pub->delete_ = fiasco_d_options_delete;
    pub->set_smoothing = fiasco_d_options_set_smoothing;
    pub->set_magnification = fiasco_d_options_set_magnification;
    pub->set_4_2_0_format = fiasco_d_options_set_4_2_0_format;
    strcpy(o->id, "DOFIASCO");
    o->smoothing = 70;
    return pub;
}

void fiasco_d_options_delete(fiasco_d_options_t *options)
{
    d_options *o = cast_d_options(options);
    if (!o) return;
    o->id[0] = 0;
    free(o);
    free(options);
}

int fiasco_d_options_set_smoothing(fiasco_d_options_t *options, int smoothing)
{
    d_options *o = cast_d_options(options);
    if (!o) return 0;
    if (smoothing < -1 || smoothing > 100) { fa_set_error("Smoothing percentage must be in the range [-1, 100]."); return 0; }
    o->smoothing = smoothing;
    return 1;
}

int fiasco_d_options_set_magnification(fiasco_d_options_t *options, int level)
{
    d_options *o = cast_d_options(options);
    if (!o) return 0;
    o->magnification = level;
    return 1;
}

int fiasco_d_options_set_4_2_0_format(fiasco_d_options_t *options, int format)
{
    d_options *o = cast_d_options(options);
    if (!o) return 0;
    o->format_420 = format != 0;
    return 1;
}

/* ---------------------------------------------------------------- images (lib/image.c:57-174) */

/* The buffers of a decoder's images that went, for its next frames: an image gives its planes back here instead of
 * freeing them, and the outlet takes them before it allocates (fa_outlet.take), so a decoder that is played at a steady
 * pace allocates as many buffers as its caller holds images at once.  Shared by the decoder and its images, which may
 * outlive it (refs); once the decoder went (alive == 0) buffers are freed.  Images may be deleted on other threads */
enum { POOL_MAX = 64 };
typedef struct d_pool {
    pthread_mutex_t mu;
    int      refs, alive;
    unsigned n;
    void    *buf[POOL_MAX];
    size_t   bytes[POOL_MAX];
    int      dev[POOL_MAX];
} d_pool;

static d_pool *pool_new(void)
{
    d_pool *p = (d_pool *) calloc(1, sizeof *p);
    if (!p) return NULL;
    pthread_mutex_init(&p->mu, NULL);
    p->refs = 1; p->alive = 1;
    return p;
}

static void pool_unref(d_pool *p)
{
    int last;
    if (!p) return;
    pthread_mutex_lock(&p->mu);
    last = --p->refs == 0;
    pthread_mutex_unlock(&p->mu);
    if (last) { pthread_mutex_destroy(&p->mu); free(p); }
}

/* fa_outlet.take */
static void *pool_take(void *pool, size_t bytes, int device)
{
    d_pool *p = (d_pool *) pool;
    void *got = NULL;
    unsigned i;
    pthread_mutex_lock(&p->mu);
    for (i = 0; i < p->n && !got; i++)
        if (p->bytes[i] == bytes && p->dev[i] == device) {
            got = p->buf[i];
            p->n--;
            p->buf[i] = p->buf[p->n]; p->bytes[i] = p->bytes[p->n]; p->dev[i] = p->dev[p->n];
        }
    pthread_mutex_unlock(&p->mu);
    return got;
}

/* the planes of an image that goes */
static void pool_give(d_pool *p, void *buf, size_t bytes, int device)
{
    int kept = 0;
    if (p) {
        pthread_mutex_lock(&p->mu);
        if (p->alive && p->n < POOL_MAX) { p->buf[p->n] = buf; p->bytes[p->n] = bytes; p->dev[p->n] = device; p->n++; kept = 1; }
        pthread_mutex_unlock(&p->mu);
    }
    if (!kept) fa_dev_free(buf, device);
}

/* the decoder goes: what the pool holds is freed, what its images still hold is freed when they go */
static void pool_close(d_pool *p)
{
    unsigned i, n;
    if (!p) return;
    pthread_mutex_lock(&p->mu);
    p->alive = 0; n = p->n; p->n = 0;
    pthread_mutex_unlock(&p->mu);
    for (i = 0; i < n; i++) fa_dev_free(p->buf[i], p->dev[i]);
    pool_unref(p);
}

/* the planes of an image: in device memory (a decoded frame, or an uploaded file), on the host (a file), or both */
typedef struct d_image {
    char      id[9];
    unsigned  width, height;
    int       color, format_420;
    size_t    vals;               /* of all planes */
    int16_t  *dev;                /* Y / Cb / Cr back to back on device dev_id, or NULL */
    int       dev_id;
    fa_image *host;               /* fiasco_image_new: the planes of the file, or NULL */
    d_pool   *pool;               /* a decoded frame: where dev goes when the image does, or NULL */
} d_image;

static d_image *cast_image(const fiasco_image_t *image)
{
    d_image *im = image ? (d_image *) image->private_ : NULL;
    if (!im) { fa_set_error("Parameter `%s' not defined (NULL).", "image"); return NULL; }
    if (strcmp(im->id, "IFIASCO")) { fa_set_error("Parameter `image' doesn't match required type."); return NULL; }
    return im;
}

static fiasco_image_t *image_handle(d_image *im)
{
    fiasco_image_t *pub = (fiasco_image_t *) fiasco_calloc(1, sizeof *pub);
    if (!pub) { fa_set_error("Out of memory."); return NULL; }
    strcpy(im->id, "IFIASCO");
    pub->private_ = im;
    pub->delete_ = fiasco_image_delete;
    pub->get_width = fiasco_image_get_width;
    pub->get_height = fiasco_image_get_height;
    pub->is_color = fiasco_image_is_color;
    return pub;
}

static void image_release(d_image *im)
{
    if (!im) return;
    if (im->dev && im->pool) pool_give(im->pool, im->dev, im->vals * 2, im->dev_id);
    else if (im->dev) fa_dev_free(im->dev, im->dev_id);
    pool_unref(im->pool);
    fa_image_free(im->host);
    im->id[0] = 0;
    free(im);
}

fiasco_image_t *fiasco_image_new(const char *filename)
{
    size_t len = 0;
    const char *name = filename && strcmp(filename, "-") ? filename : NULL;
    unsigned char *data = fa_read_whole_file(name, "FIASCO_IMAGES", &len);
    d_image *im;
    fiasco_image_t *pub;
    if (!data) return NULL;
    im = (d_image *) calloc(1, sizeof *im);
    if (!im) { free(data); fa_set_error("Out of memory."); return NULL; }
    im->host = fa_image_from_pnm(data, len, name ? name : "stdin");
    free(data);
    if (!im->host) { free(im); return NULL; }
    im->width = im->host->width; im->height = im->host->height; im->color = im->host->color;
    im->vals = (size_t) im->width * im->height * (im->color ? 3 : 1);
    pub = image_handle(im);
    if (!pub) image_release(im);
    return pub;
}

void fiasco_image_delete(fiasco_image_t *image)
{
    d_image *im = cast_image(image);
    if (!im) return;
    image_release(im);
    free(image);
}

unsigned fiasco_image_get_width(fiasco_image_t *image) { d_image *im = cast_image(image); return im ? im->width : 0; }
/* the reference returns the WIDTH here (lib/image.c:127-135), and so does this; the height: fiasco_amd_image_get_height() */
unsigned fiasco_image_get_height(fiasco_image_t *image) { d_image *im = cast_image(image); return im ? im->width : 0; }
unsigned fiasco_amd_image_get_height(const fiasco_image_t *image) { d_image *im = cast_image(image); return im ? im->height : 0; }
int fiasco_image_is_color(fiasco_image_t *image) { d_image *im = cast_image(image); return im ? im->color : 0; }
int fiasco_amd_image_format(const fiasco_image_t *image) { d_image *im = cast_image(image); return im ? im->format_420 : -1; }

int fiasco_amd_image_planes(const fiasco_image_t *image, int16_t *out)
{
    d_image *im = cast_image(image);
    const size_t npix = im ? (size_t) im->width * im->height : 0;
    int b;
    if (!im) return 0;
    if (!out) { fa_set_error("fiasco_amd_image_planes: no place for the planes"); return 0; }
    if (im->host) {
        for (b = 0; b < (im->color ? 3 : 1); b++) memcpy(out + b * npix, im->host->pixels[b], npix * 2);
        return 1;
    }
    return fa_dev_download(out, im->dev, im->vals * 2, im->dev_id);
}

int fiasco_amd_image_planes_device(const fiasco_image_t *image, const int16_t *planes[3], int *device)
{
    d_image *im = cast_image(image);
    const size_t npix = im ? (size_t) im->width * im->height : 0;
    const size_t cpix = im && im->format_420 ? (size_t) (im->width >> 1) * (im->height >> 1) : npix;
    if (!im) return 0;
    if (!planes) { fa_set_error("fiasco_amd_image_planes_device: no place for the planes"); return 0; }
    if (!im->dev) {
        /* an image that was read from a file: its planes back to back, uploaded once */
        int16_t *all = (int16_t *) malloc(im->vals * 2);
        int b;
        if (!all) { fa_set_error("Out of memory."); return 0; }
        for (b = 0; b < (im->color ? 3 : 1); b++) memcpy(all + b * npix, im->host->pixels[b], npix * 2);
        im->dev = (int16_t *) fa_dev_upload(all, im->vals * 2, &im->dev_id);
        free(all);
        if (!im->dev) return 0;
    }
    planes[0] = im->dev;
    planes[1] = im->color ? im->dev + npix : NULL;
    planes[2] = im->color ? im->dev + npix + cpix : NULL;
    if (device) *device = im->dev_id;
    return 1;
}

/* ---------------------------------------------------------------- the decoder (codec/dfiasco.c) */

typedef struct d_decoder {
    char       id[9];
    struct fiasco_amd_stream *stream;
    int        magnify, smoothing, format_420;
    unsigned   n, display;          /* display frames; the next one handed out */
    unsigned   read_ahead;
    fa_cursor *cursor;              /* opened by the first frame, at the display frame it is called for */
    int        cursor_420;
    int16_t  **ready;               /* [n] by display number: the shown planes of frames decoded and not handed out yet */
    int       *ready_dev;           /* [n] */
    d_pool    *pool;                /* the buffers of images that went, for the frames to come */
    void      *keep;                /* the share's stream, events and arena, kept between calls (fa_outlet.keep) */
    void      *pixels;              /* write_frame: the 8-bit pixels in device memory, kept */
    size_t     pixels_cap;
    int        pixels_dev;
} d_decoder;

static d_decoder *cast_decoder(const fiasco_decoder_t *decoder)
{
    d_decoder *d = decoder ? (d_decoder *) decoder->private_ : NULL;
    if (!d) { fa_set_error("Parameter `%s' not defined (NULL).", "dfiasco"); return NULL; }
    if (strcmp(d->id, "DFIASCO")) { fa_set_error("Parameter `dfiasco' doesn't match required type."); return NULL; }
    return d;
}

static void drop_cursor(d_decoder *d)
{
    unsigned i;
    fa_cursor_close(d->cursor);
    d->cursor = NULL;
    for (i = 0; d->ready && i < d->n; i++) if (d->ready[i]) { fa_dev_free(d->ready[i], d->ready_dev[i]); d->ready[i] = NULL; }
}

static void decoder_release(d_decoder *d)
{
    if (!d) return;
    drop_cursor(d);
    fa_dev_keep_free(d->keep);
    pool_close(d->pool);
    if (d->pixels) fa_dev_free(d->pixels, d->pixels_dev);
    free(d->ready); free(d->ready_dev);
    fiasco_amd_stream_free(d->stream);
    d->id[0] = 0;
    free(d);
}

/* the limits of fiasco_decoder_new (codec/dfiasco.c:104-137), with its sentences */
static int check_magnification(const fa_info *wi, int m)
{
    int n;
    if (m >= 0) {
        const unsigned long pixels = (unsigned long) wi->width * wi->height;
        for (n = 1; n <= m; n++)
            if (pixels << (n << 1) > 2048ul * 2048ul) {            /* stops at n <= 12: the shift stays small */
                fa_set_error("Magnifaction factor `%d' is too large. Maximium value is %d.", m, n - 1 > 0 ? n - 1 : 0);
                return 0;
            }
    } else {
        for (n = 0; n <= -(long) m; n++)
            if (wi->width >> n < 32 || wi->height >> n < 32) {     /* stops at n <= 27 */
                fa_set_error("Magnifaction factor `%d' is too small. Minimum value is %d.", m, -(n - 1 > 0 ? n - 1 : 0));
                return 0;
            }
    }
    return 1;
}

static fiasco_decoder_t *decoder_of(struct fiasco_amd_stream *s, const fiasco_d_options_t *options)
{
    const d_options *o = options ? cast_d_options(options) : NULL;
    const fa_info *wi;
    d_decoder *d;
    fiasco_decoder_t *pub;
    unsigned w, h;
    if (!s || (options && !o)) { fiasco_amd_stream_free(s); return NULL; }
    wi = fa_stream_info(s);
    d = (d_decoder *) calloc(1, sizeof *d);
    pub = (fiasco_decoder_t *) fiasco_calloc(1, sizeof *pub);
    if (d) { d->ready = (int16_t **) calloc(wi->frames ? wi->frames : 1, sizeof *d->ready); d->ready_dev = (int *) calloc(wi->frames ? wi->frames : 1, sizeof *d->ready_dev); d->pool = pool_new(); }
    if (!d || !pub || !d->ready || !d->ready_dev || !d->pool) {
        if (d) { free(d->ready); free(d->ready_dev); pool_unref(d->pool); }
        free(d); free(pub); fiasco_amd_stream_free(s);
        fa_set_error("Out of memory.");
        return NULL;
    }
    strcpy(d->id, "DFIASCO");
    d->stream = s; d->n = wi->frames; d->read_ahead = 32;
    d->smoothing = o ? o->smoothing : 70; d->magnify = o ? o->magnification : 0; d->format_420 = o ? o->format_420 : 0;
    /* the reference's limits first, then what this library's frames can be (fiasco_amd_magnified_size) */
    if (!check_magnification(wi, d->magnify) || !fiasco_amd_magnified_size(wi->width, wi->height, d->magnify, &w, &h)) {
        decoder_release(d); free(pub);
        return NULL;
    }
    pub->private_ = d;
    pub->delete_ = fiasco_decoder_delete;
    pub->write_frame = fiasco_decoder_write_frame;
    pub->get_frame = fiasco_decoder_get_frame;
    pub->get_length = fiasco_decoder_get_length;
    pub->get_rate = fiasco_decoder_get_rate;
    pub->get_width = fiasco_decoder_get_width;
    pub->get_height = fiasco_decoder_get_height;
    pub->get_title = fiasco_decoder_get_title;
    pub->get_comment = fiasco_decoder_get_comment;
    pub->is_color = fiasco_decoder_is_color;
    return pub;
}

fiasco_decoder_t *fiasco_decoder_new(const char *filename, const fiasco_d_options_t *options)
{
    const char *name = filename && strcmp(filename, "-") ? filename : NULL;
    size_t len = 0;
    unsigned char *data;
    struct fiasco_amd_stream *s;
    if (options && !cast_d_options(options)) return NULL;
    data = fa_read_whole_file(name, "FIASCO_DATA", &len);
    if (!data) return NULL;
    s = fa_stream_open_named(data, len, name ? name : "stdin");
    free(data);
    return decoder_of(s, options);
}

fiasco_decoder_t *fiasco_amd_decoder_new_memory(const unsigned char *data, size_t len, const fiasco_d_options_t *options)
{
    if (!data) { fa_set_error("fiasco_amd_decoder_new_memory: no stream"); return NULL; }
    if (options && !cast_d_options(options)) return NULL;
    return decoder_of(fa_stream_open_named(data, len, "<memory>"), options);
}

int fiasco_decoder_delete(fiasco_decoder_t *decoder)
{
    d_decoder *d = cast_decoder(decoder);
    if (!d) return 1;
    decoder_release(d);
    free(decoder);
    return 1;
}

int fiasco_amd_decoder_position(const fiasco_decoder_t *decoder)
{
    d_decoder *d = cast_decoder(decoder);
    return d ? (int) d->display : -1;
}

int fiasco_amd_decoder_set_read_ahead(fiasco_decoder_t *decoder, unsigned n)
{
    d_decoder *d = cast_decoder(decoder);
    if (!d) return 0;
    if (!n) { fa_set_error("fiasco_amd_decoder_set_read_ahead: at least the frame asked for is decoded (n >= 1)"); return 0; }
    d->read_ahead = n;
    return 1;
}

/* get_next_frame for a caller: the next display frame in `format_420' as an image that owns its planes; NULL + message.
 * A frame that fails is consumed; a call that is refused as a whole (no device, past the end, a stream the walk refuses)
 * consumes nothing */
static d_image *next_frame(d_decoder *d, const char *who, int format_420)
{
    const fa_info *wi = fa_stream_info(d->stream);
    const int fmt = format_420 != 0;
    fa_outlet outlet;
    const char *cause = "";
    unsigned disp, w = 0, h = 0;
    size_t vals;
    d_image *im;
    if (d->display >= d->n) { fa_set_error("%s: no such frame: the stream has %u frames", who, d->n); return NULL; }
    /* the reference shrinks EVERY state of a gray automaton by a level here, the initial basis included (enlarge_image,
     * codec/decoder.c:796-800 with y_root == -1): refused as the stream entries refuse it */
    if (fmt && !wi->color) { fa_set_error("%s: 4:2:0: a gray frame has no chroma bands", who); return NULL; }
    if (!fa_dev_available()) return NULL;
    if (d->cursor && d->cursor_420 != fmt) drop_cursor(d);
    if (!d->cursor) {
        d->cursor = fa_cursor_open(d->stream, who, d->display, d->n - d->display, NULL, d->magnify, d->smoothing, fmt, 0);
        d->cursor_420 = fmt;
        if (!d->cursor) return NULL;
    }
    if (!fiasco_amd_magnified_size(wi->width, wi->height, d->magnify, &w, &h)) return NULL;
    disp = d->display++;
    vals = fmt ? (size_t) w * h + 2 * ((size_t) (w >> 1) * (h >> 1)) : (size_t) w * h * (wi->color ? 3 : 1);
    outlet.planes = d->ready; outlet.device = d->ready_dev;
    outlet.bytes = vals * 2; outlet.take = pool_take; outlet.pool = d->pool; outlet.keep = &d->keep;
    fa_cursor_advance(d->cursor, disp, d->read_ahead, fa_dev_outlet_run, &outlet);
    if (fa_cursor_status(d->cursor, disp, &cause) != 1 || !d->ready[disp]) {
        if (d->ready[disp]) { fa_dev_free(d->ready[disp], d->ready_dev[disp]); d->ready[disp] = NULL; }
        fa_set_error("%s: display frame %u: %s", who, disp, cause[0] ? cause : "the frame was not decoded");
        return NULL;
    }
    im = (d_image *) calloc(1, sizeof *im);
    if (!im) { fa_set_error("Out of memory."); return NULL; }       /* the planes stay the decoder's, released with it */
    strcpy(im->id, "IFIASCO");
    im->width = w; im->height = h; im->color = wi->color; im->format_420 = fmt;
    im->vals = vals;
    im->dev = d->ready[disp]; im->dev_id = d->ready_dev[disp];
    pthread_mutex_lock(&d->pool->mu); d->pool->refs++; pthread_mutex_unlock(&d->pool->mu);
    im->pool = d->pool;
    d->ready[disp] = NULL;
    return im;
}

fiasco_image_t *fiasco_decoder_get_frame(fiasco_decoder_t *decoder)
{
    d_decoder *d = cast_decoder(decoder);
    d_image *im = d ? next_frame(d, "fiasco_decoder_get_frame", d->format_420) : NULL;
    fiasco_image_t *pub = im ? image_handle(im) : NULL;
    if (im && !pub) image_release(im);
    return pub;
}

/* write_image (lib/image.c:394-415): the pixels of the plane-to-pixel kernel behind the PNM header */
int fiasco_decoder_write_frame(fiasco_decoder_t *decoder, const char *filename)
{
    d_decoder *d = cast_decoder(decoder);
    d_image *im = d ? next_frame(d, "fiasco_decoder_write_frame", 0) : NULL;
    const char *name = filename && strcmp(filename, "-") ? filename : NULL;
    fiasco_amd_device_target t;
    unsigned char *host = NULL;
    size_t bytes;
    FILE *f = NULL;
    int ok = 0;
    if (!im) return 0;
    bytes = (size_t) im->width * im->height * (im->color ? 3 : 1);
    memset(&t, 0, sizeof t);
    if (d->pixels && d->pixels_dev != im->dev_id) { fa_dev_free(d->pixels, d->pixels_dev); d->pixels = NULL; d->pixels_cap = 0; }
    if (!fa_dev_reserve(&d->pixels, &d->pixels_cap, bytes, im->dev_id)) goto done;
    d->pixels_dev = im->dev_id;
    t.data = d->pixels; t.width = im->width; t.height = im->height; t.layout = im->color ? FIASCO_AMD_RGB8_INTERLEAVED : FIASCO_AMD_GRAY8;
    host = (unsigned char *) malloc(bytes);
    if (!host) { fa_set_error("Out of memory."); goto done; }
    if (!fiasco_amd_planes_to_pixels_device(im->dev, im->color, &t, NULL) || !fa_dev_download(host, d->pixels, bytes, im->dev_id)) goto done;
    f = open_file(name, "FIASCO_IMAGES", WRITE_ACCESS);
    if (!f) { fa_set_error("File `%s': I/O Error - %s.", name ? name : "stdout", strerror(errno)); goto done; }
    fprintf(f, "%s\n%d %d\n255\n", im->color ? "P6" : "P5", (int) im->width, (int) im->height);
    if (fwrite(host, 1, bytes, f) != bytes) { fa_set_error("Can't write image pixel %d.", 0); goto done; }
    ok = 1;
done:
    if (f && f != stdout) { if (fclose(f) && ok) { fa_set_error("File `%s': I/O Error - %s.", name, strerror(errno)); ok = 0; } }
    else if (f) fflush(f);
    free(host);
    image_release(im);
    return ok;
}

unsigned fiasco_decoder_get_length(fiasco_decoder_t *decoder) { d_decoder *d = cast_decoder(decoder); return d ? fa_stream_info(d->stream)->frames : 0; }
unsigned fiasco_decoder_get_rate(fiasco_decoder_t *decoder) { d_decoder *d = cast_decoder(decoder); return d ? fa_stream_info(d->stream)->fps : 0; }
int fiasco_decoder_is_color(fiasco_decoder_t *decoder) { d_decoder *d = cast_decoder(decoder); return d ? fa_stream_info(d->stream)->color : 0; }

/* the side length shown, rounded up to even (codec/dfiasco.c:228-266) */
static unsigned shown_side(unsigned side, int m)
{
    const unsigned v = m >= 0 ? side << m : side >> -m;
    return v & 1 ? v + 1 : v;
}

unsigned fiasco_decoder_get_width(fiasco_decoder_t *decoder)
{
    d_decoder *d = cast_decoder(decoder);
    return d ? shown_side(fa_stream_info(d->stream)->width, d->magnify) : 0;
}

unsigned fiasco_decoder_get_height(fiasco_decoder_t *decoder)
{
    d_decoder *d = cast_decoder(decoder);
    return d ? shown_side(fa_stream_info(d->stream)->height, d->magnify) : 0;
}

const char *fiasco_decoder_get_title(fiasco_decoder_t *decoder)
{
    d_decoder *d = cast_decoder(decoder);
    const char *t = d ? fa_stream_info(d->stream)->title : NULL;
    return d ? (t ? t : "") : NULL;
}

const char *fiasco_decoder_get_comment(fiasco_decoder_t *decoder)
{
    d_decoder *d = cast_decoder(decoder);
    const char *t = d ? fa_stream_info(d->stream)->comment : NULL;
    return d ? (t ? t : "") : NULL;
}

/* ---------------------------------------------------------------- the renderer (lib/dither.c) */

/* the renderer of libfiasco_amd_render.h and the staging surface in device memory it renders device images into: the
 * surface makes a renderer an object for one thread at a time */
typedef struct d_renderer {
    fiasco_amd_renderer_t *r;
    void   *surface;
    size_t  surface_cap;
    int     surface_dev;
} d_renderer;

fiasco_renderer_t *fiasco_renderer_new(unsigned long red_mask, unsigned long green_mask, unsigned long blue_mask, unsigned bpp,
                                       int double_resolution)
{
    fiasco_amd_renderer_t *r = fiasco_amd_renderer_new(red_mask, green_mask, blue_mask, bpp, double_resolution);
    d_renderer *p = r ? (d_renderer *) calloc(1, sizeof *p) : NULL;
    fiasco_renderer_t *pub = p ? (fiasco_renderer_t *) fiasco_calloc(1, sizeof *pub) : NULL;
    if (!r) return NULL;
    if (!p || !pub) { free(p); fiasco_amd_renderer_delete(r); fa_set_error("Out of memory."); return NULL; }
    p->r = r;
    pub->private_ = p;
    pub->render = fiasco_renderer_render;
    pub->delete_ = fiasco_renderer_delete;
    return pub;
}

void fiasco_renderer_delete(fiasco_renderer_t *renderer)
{
    d_renderer *p = renderer ? (d_renderer *) renderer->private_ : NULL;
    if (!renderer) { fa_set_error("Parameter `%s' not defined (NULL).", "renderer"); return; }
    if (p) {
        if (p->surface) fa_dev_free(p->surface, p->surface_dev);
        fiasco_amd_renderer_delete(p->r);
        free(p);
    }
    free(renderer);
}

/* the size of the surface the image renders into; 0 + the refusal of libfiasco_amd_render[_420].h */
static int surface_of(const d_renderer *p, const d_image *im, fiasco_amd_device_surface *s, size_t *bytes)
{
    size_t row = 0;
    memset(s, 0, sizeof *s);
    if (im->format_420 ? !fiasco_amd_renderer_surface_size_420(p->r, im->width, im->height, &s->width, &s->height, &row)
                       : !fiasco_amd_renderer_surface_size(p->r, im->width, im->height, im->color, &s->width, &s->height, &row)) return 0;
    *bytes = row * s->height;
    return 1;
}

static int render_on_device(const d_renderer *p, const d_image *im, const fiasco_amd_device_surface *s, void *stream)
{
    const size_t npix = (size_t) im->width * im->height, cpix = (size_t) (im->width >> 1) * (im->height >> 1);
    if (im->format_420) return fiasco_amd_planes_render_device_420(im->dev, im->dev + npix, im->dev + npix + cpix, im->width, im->height, p->r, s, stream);
    return fiasco_amd_planes_render_device(im->dev, im->color, im->width, im->height, p->r, s, stream);
}

int fiasco_renderer_render(const fiasco_renderer_t *renderer, unsigned char *ximage, const fiasco_image_t *fiasco_image)
{
    d_renderer *p = renderer ? (d_renderer *) renderer->private_ : NULL;
    d_image *im;
    fiasco_amd_device_surface s;
    size_t bytes = 0;
    if (!p) { fa_set_error("Parameter `%s' not defined (NULL).", "this"); return 0; }
    if (!ximage) { fa_set_error("Parameter `%s' not defined (NULL).", "ximage"); return 0; }
    if (!fiasco_image) { fa_set_error("Parameter `%s' not defined (NULL).", "fiasco_image"); return 0; }
    im = cast_image(fiasco_image);
    if (!im || !surface_of(p, im, &s, &bytes)) return 0;
    if (!im->dev) {
        /* an image that was read from a file, in host memory: the host loops (fa_render.c) */
        const size_t npix = (size_t) im->width * im->height;
        int16_t *all = (int16_t *) malloc(im->vals * 2);
        int b, ok;
        if (!all) { fa_set_error("Out of memory."); return 0; }
        for (b = 0; b < (im->color ? 3 : 1); b++) memcpy(all + b * npix, im->host->pixels[b], npix * 2);
        ok = fiasco_amd_renderer_render_planes(p->r, all, im->color, im->width, im->height, ximage);
        free(all);
        return ok;
    }
    if (p->surface && p->surface_dev != im->dev_id) { fa_dev_free(p->surface, p->surface_dev); p->surface = NULL; p->surface_cap = 0; }
    if (!fa_dev_reserve(&p->surface, &p->surface_cap, bytes, im->dev_id)) return 0;
    p->surface_dev = im->dev_id;
    s.data = p->surface;
    return render_on_device(p, im, &s, NULL) && fa_dev_download(ximage, p->surface, bytes, im->dev_id);
}

int fiasco_amd_renderer_render_device(const fiasco_renderer_t *renderer, const fiasco_amd_device_surface *surface, const fiasco_image_t *image,
                                      void *hip_stream)
{
    d_renderer *p = renderer ? (d_renderer *) renderer->private_ : NULL;
    d_image *im;
    const int16_t *planes[3];
    if (!p) { fa_set_error("Parameter `%s' not defined (NULL).", "this"); return 0; }
    if (!surface || !surface->data) { fa_set_error("Parameter `%s' not defined (NULL).", "surface"); return 0; }
    if (!image) { fa_set_error("Parameter `%s' not defined (NULL).", "fiasco_image"); return 0; }
    im = cast_image(image);
    if (!im || !fiasco_amd_image_planes_device(image, planes, NULL)) return 0;
    return render_on_device(p, im, surface, hip_stream);
}
