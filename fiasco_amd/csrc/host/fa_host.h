/*
 *  fa_host.h -- internal host-side declarations of libfiasco_amd.
 *
 *  Host C keeps what the reference keeps around the hot path: options object, PNM input,
 *  basis automaton, frame driver and the .fco stream writer.  Everything from
 *  subdivide() downwards (partition search, matching pursuit, inner-product tables,
 *  rate models) lives behind fa_core_encode_frames(), which is implemented
 *    - by the HIP device coder (csrc/hip/core_hip.cpp) in the product library, and
 *    - by the CPU restatement (oracle/oracle_core.c) in the test-only oracle library.
 */
#ifndef FA_HOST_H
#define FA_HOST_H

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include "libfiasco_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_MAXEDGES      5     /* reference codec/wfa.h:20 */
#define FA_MAXLABELS     2     /* reference codec/wfa.h:22 */
#define FA_STOCK_STATES  6000  /* reference codec/wfa.h:21 */
#define FA_STOCK_LEVEL   22    /* reference codec/wfa.h:23 */
#define FA_CAP_STATES    32000 /* word_t state ids */
#define FA_CAP_LEVEL     26
#define FA_NO_EDGE       (-1)
#define FA_RANGE         (-1)
#define FA_MAXCOSTS      1e20f /* reference codec/coder.c:53 */
#define FA_USE_DOMAIN    2     /* reference codec/wfa.h:41 USE_DOMAIN_MASK */
#define FA_AUXILIARY     1

enum { FA_I_FRAME = 0, FA_P_FRAME = 1, FA_B_FRAME = 2 };
enum { FA_GRAY = 0, FA_Y = 0, FA_CB = 1, FA_CR = 2 };

/* level geometry, reference lib/macros.h:48-52 */
#define fa_width_of_level(l)   (1u << ((l) >> 1))
#define fa_height_of_level(l)  (1u << (((l) + 1) >> 1))
#define fa_size_of_level(l)    (1u << (l))
#define fa_address_of_level(l) (fa_size_of_level(l) - 1u)
#define fa_size_of_tree(l)     (fa_address_of_level((l) + 1))

/* ---------------- error / messages (reference lib/error.c) ---------------- */
void fa_set_error(const char *fmt, ...);
/* getenv() for developer / test switches: null unless FIASCO_AMD_DEBUG is set (core_hip.cpp; the oracle's
 * core has its own) */
const char *fa_knob(const char *name);
void fa_warning(const char *fmt, ...);
void fa_message(const char *fmt, ...);
void fa_debug(const char *fmt, ...);
void fa_progress(const char *fmt, ...);

/* ---------------- host threads (fa_threads.c) ---------------- */
#define FA_FAN_MAX 32
unsigned fa_online_cpus(void);   /* sysconf(_SC_NPROCESSORS_ONLN), at least 1 */
/* share(ctx, t, nt) for t = 0 .. nt - 1, nt clamped to 1 .. FA_FAN_MAX: share 0 on the caller, the others on threads (on
 * the caller where no thread starts); returns when all are done.  A share takes items t, t + nt, ... and leaves what
 * the caller needs of it in arrays of ctx indexed by t */
void fa_fan_out(unsigned nt, void (*share)(void *ctx, unsigned t, unsigned nt), void *ctx);

/* ---------------- reduced precision format (reference lib/rpf.h) ---------------- */
typedef struct fa_rpf {
    unsigned mantissa_bits;
    float    range;
    int      range_e;
} fa_rpf;
void fa_rpf_init(fa_rpf *r, unsigned mantissa, int range_e);
int  fa_rtob(float f, const fa_rpf *r);   /* used by the stream writer (weights) */
float fa_btor(int binary, const fa_rpf *r); /* used by the stream reader: 0 <= binary < 2^(mantissa_bits + 1) */

/* ---------------- options (reference codec/options.h:20-65) ---------------- */
typedef struct fa_options {
    char     id[9];
    char    *basis_name;
    unsigned lc_min_level, lc_max_level;
    unsigned p_min_level, p_max_level;
    unsigned images_level;
    unsigned max_states, chroma_max_states, max_elements;
    unsigned tiling_exponent;
    int      tiling_method;
    char    *id_domain_pool, *id_d_domain_pool, *id_rpf_model, *id_d_rpf_model;
    unsigned rpf_mantissa;      int rpf_range;
    unsigned dc_rpf_mantissa;   int dc_rpf_range;
    unsigned d_rpf_mantissa;    int d_rpf_range;
    unsigned d_dc_rpf_mantissa; int d_dc_rpf_range;
    float    chroma_decrease;
    int      prediction, delta_domains, normal_domains;
    unsigned search_range, fps;
    char    *pattern;
    int      half_pixel_prediction, cross_B_search, B_as_past_ref;
    int      check_for_underflow, check_for_overflow, second_domain_block, full_search;
    int      progress_meter;
    char    *title, *comment;
    unsigned smoothing;
} fa_options;
fa_options *fa_cast_options(const fiasco_c_options_t *o);

/* ---------------- image (reference lib/image.h, 12.4 fixed point int16) ---------- */
typedef struct fa_image {
    unsigned width, height;
    int      color;
    int16_t *pixels[3];
    int      borrowed;       /* planes belong to somebody else (upload staging buffer) */
    void    *dev;            /* decoded frames: the same planes [bands][height][width] on device dev_id, or NULL
                                (fa_core_decode_frames; released by fa_image_free through fa_core_release_dev) */
    int      dev_id;
    /* frames that were handed over in device memory (fiasco_amd_batch_stage_device / _upload_device): the converted
     * planes [bands][height][width] inside the core's input buffer on device src_dev_id, borrowed.  Such a frame
     * has no host planes (pixels[] NULL) until somebody asks for them: fa_image_host_planes() */
    const int16_t *src_dev;
    int      src_dev_id;
    void    *src_owner;      /* the core's handle of the share that holds src_dev */
} fa_image;
/* parse raw P5/P6 from memory; returns NULL + error message on failure */
fa_image *fa_image_from_pnm(const unsigned char *buf, size_t len, const char *name);
fa_image *fa_image_from_pnm_into(const unsigned char *buf, size_t len, const char *name,
                                 unsigned want_w, unsigned want_h, int want_color, int16_t *planes);
int       fa_pnm_header(const unsigned char *buf, size_t len, const char *name,
                        unsigned *w, unsigned *h, int *color, size_t *data_off);
void      fa_image_free(fa_image *im);
fa_image *fa_image_alloc(unsigned width, unsigned height, int color);   /* zeroed planes */
/* the geometry rules of read_pnmheader / read_image (lib/image.c:194-195, :316-323) for a frame that does not come
 * from a PNM header; 0 + the reader's message */
int       fa_image_check_size(unsigned width, unsigned height, const char *name);
/* Frames that are YCbCr already (include/libfiasco_amd_ycbcr.h).  fa_ycbcr_check: everything that can be said about
 * frame i without asking where its memory lies -- the planes, c_step, subsampling, the size, the pitches; *out: the
 * frame with its pitches filled in; 0 + message.  fa_image_from_ycbcr: a checked frame in host memory as planes,
 * (byte - 128) * 16, a 4:2:0 chroma sample replicated over its 2 x 2 pixels; planes: NULL (the image owns its planes),
 * or where the three bands go back to back (borrowed, as fa_image_from_pnm_into). */
struct fiasco_amd_ycbcr_frame;
int       fa_ycbcr_check(unsigned i, const struct fiasco_amd_ycbcr_frame *in, struct fiasco_amd_ycbcr_frame *out);
fa_image *fa_image_from_ycbcr(const struct fiasco_amd_ycbcr_frame *f, int16_t *planes);
/* Host planes on demand.  The host never reads input pixels while it encodes; only the decoded-PSNR calls and
 * fiasco_amd_batch_input_planes() do.  For a frame that lives on the device the planes are allocated here and
 * filled by fa_image_fetch, which the product's core sets (the host C names no core function: the test oracle
 * links the same files).  1 ok / 0 + message. */
extern int (*fa_image_fetch)(fa_image *im);
int       fa_image_host_planes(const fa_image *im);

/* ---------------- reconstruction (reference codec/decoder.c, codec/motion.c) ------- */
unsigned char *fa_read_whole_file(const char *name, const char *env_var, size_t *len);

/* ---------------- automaton container handed to the writer ---------------- */
/* motion vector of a (state, label): reference codec/wfa.h:43-63 mv_t */
enum { FA_MV_NONE = 0, FA_MV_FORWARD = 1, FA_MV_BACKWARD = 2, FA_MV_INTERPOLATED = 3 };
typedef struct fa_mv { int16_t type, fx, fy, bx, by; } fa_mv;

typedef struct fa_wfa {
    unsigned cap;                 /* allocated states */
    unsigned states, basis_states, root_state;
    int      frame_type;
    float   *final_distribution;  /* [cap] */
    uint8_t *level_of_state;      /* [cap] */
    uint8_t *domain_type;         /* [cap] */
    uint8_t *delta_state;         /* [cap] */
    int16_t *tree;                /* [cap][2] */
    uint16_t *x, *y;              /* [cap][2] */
    int16_t *into;                /* [cap][2][6] */
    float   *weight;              /* [cap][2][6] */
    int16_t *y_state;             /* [cap][2] */
    uint8_t *y_column;            /* [cap][2] */
    uint8_t *prediction;          /* [cap][2] */
    fa_mv   *mv;                  /* [cap][2] mv_tree */
} fa_wfa;
#define FA_TREE(w, s, l)      ((w)->tree[(s) * 2 + (l)])
#define FA_INTO(w, s, l, e)   ((w)->into[((s) * 2 + (l)) * 6 + (e)])
#define FA_WEIGHT(w, s, l, e) ((w)->weight[((s) * 2 + (l)) * 6 + (e)])
fa_wfa *fa_wfa_alloc(unsigned cap);
void    fa_wfa_free(fa_wfa *w);
void    fa_wfa_remove_states(fa_wfa *w, unsigned from);
int     fa_wfa_append_edge(fa_wfa *w, unsigned from, unsigned into, float weight, unsigned label);
                                  /* 0: the label already has FA_MAXEDGES edges */
int     fa_load_basis(const char *name, fa_wfa *w);   /* 1 ok / 0 error */

/* TEST ORACLE ONLY (oracle/oracle_decoder.c; the product decodes on the device, fa_core_decode_frames below):
 * the frame an automaton describes, 4:4:4, cropped to the coded size (decode_image,
 * codec/decoder.c:411-536); NULL + message on failure */
fa_image *fa_decode_image(unsigned orig_width, unsigned orig_height, const fa_wfa *w, int color);
/* add the motion compensation of a P/B frame (restore_mc, codec/motion.c:37-229) */
int       fa_restore_mc(fa_image *image, const fa_image *past, const fa_image *future,
                        const fa_wfa *w, unsigned p_max_level);
void      fa_extract_mc_block(int16_t *mcblock, unsigned width, unsigned height,
                              const int16_t *reference, unsigned ref_width,
                              unsigned xo, unsigned yo, int mx, int my);
double    fa_plane_mse(const int16_t *a, const int16_t *b, size_t n);

/* the decoder as the core runs it (device library: csrc/hip/frame_decoder.inc; test oracle: the host decoder
 * above): decode_image for every job, restore_mc for the P/B frames among them (codec/coder.c:647-651) */
typedef struct fa_dec_job {
    const fa_wfa   *wfa;                  /* in  */
    unsigned        width, height;        /* in: the coded size (the decoder crops to it) */
    int             color, frame_type;    /* in  */
    const fa_image *past, *future;        /* in: references of a P/B frame */
    unsigned        p_max_level;          /* in  */
    int             skip;                 /* in: leave this job alone (keeps the index -> device dealing) */
    int             keep_dev;             /* in: leave the planes on the device too (out->dev): reference frames */
    unsigned        share_key;            /* in: as fa_job.share_key (0 = dealt by index) */
    fa_image       *out;                  /* out: the frame, or NULL + errmsg */
    char            errmsg[160];
    int             magnify;              /* in: decode at 2^magnify times the side length (dfiasco -m; intra frames; 0 = as coded).
                                           * out then has the size of fiasco_amd_magnified_size(); the test oracle does not know
                                           * the field and returns the coded size: callers check the size they get back */
    /* Consumers on the device beside `out' (the outputs of a sequence, fiasco_amd_seq_set_outputs_device): behind the
     * kernels of the job's flight the frame is written as 8-bit pixels and measured against its original, as the batch
     * entries fiasco_amd_batch_decode_device() / _decode_distortion_device() do.  The test oracle does not know the
     * fields and ignores them, as it does magnify: delivered stays 0 */
    const void     *target;               /* in: a checked fiasco_amd_device_target on the device the job is decoded on (its
                                           * data may be NULL: not written), or NULL */
    unsigned long long *sse;              /* in: [3] result slots per band on the host, or NULL */
    unsigned       *maxdiff;              /* in: [3], or NULL */
    const fa_image *orig;                 /* in: the original the frame is measured against (sse or maxdiff given) */
    void           *consumer_stream;      /* in: the caller's hipStream_t, as fiasco_amd_batch_decode_device() takes it */
    int             delivered;            /* out: 1 once every consumer the job names has had the frame */
    int             format_420;           /* in: decode in 4:2:0 (include/libfiasco_amd_420.h; fa_420_plan_of below): colour intra frames.
                                           * out then has Y at full size and, at the BEGINNING of pixels[1] and pixels[2], the packed
                                           * chroma planes of (width >> 1) x (height >> 1) values.  The test oracle does not know the field */
    int             out_420;              /* out: 1 where `out' is such a frame: callers check it as they check the size */
    int             from_stream;          /* in: a frame of a stream that is walked (fa_stream.c), whose reference frames live at the
                                           * magnification and in the format shown, as get_next_frame keeps them
                                           * (codec/decoder.c:160-410).  Lifts three refusals for P/B frames: magnify (the blocks and
                                           * vectors as enlarge_image leaves them), format_420 with keep_dev (dec_mc420_kernel; past and
                                           * future are 4:2:0 frames of the size shown) and smoothing (a frame that is smoothed AND kept
                                           * is smoothed in a copy: the next frame is predicted from the unsmoothed one).  The test
                                           * oracle does not know the field.  (Everything that fills a job is compiled against this
                                           * header and fills it by name; `smoothing' stays the last field) */
    int             smoothing;            /* in: blend the Y plane along the borders of the partition before any consumer sees the
                                           * frame (smooth_image, codec/decoder.c:674-768; csrc/hip/smooth.inc): 0 nothing, 1 .. 100
                                           * that percentage (dfiasco -s N); -1 stands for the value of the frame's stream header
                                           * (fa_info.smoothing), which the batch entries put here in its place -- a job has no
                                           * header.  Intra frames, at every magnify (the list of a magnified frame:
                                           * fa_smoothing_borders_magnified).  The test oracle does not know the field */
} fa_dec_job;
int  fa_core_decode_frames(unsigned n, fa_dec_job *jobs);    /* number of frames decoded */
/* smoothing along the partition borders (smooth_image, codec/decoder.c:674-768; fa_batch_decode.c): the borders of a
 * frame in passes (fiasco_amd_batch_smoothing_borders) */
unsigned fa_smoothing_borders(const fa_wfa *w, unsigned width, unsigned height, int color, fiasco_amd_border *out, unsigned cap);
/* ... of the frame as `dfiasco -m magnify' shows it (width x height: the coded size; fiasco_amd_batch_smoothing_borders_magnified).
 * 0 + message: the size rule refuses the magnification, or a smoothed state falls below level 1 */
unsigned fa_smoothing_borders_magnified(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out,
                                        unsigned cap);
/* 4:2:0 (include/libfiasco_amd_420.h; enlarge_image / decode_image / alloc_state_images of codec/decoder.c with
 * FORMAT_4_2_0): at magnification `magnify' a Y state is shown at its coded level + 2 magnify, a chroma state at its coded
 * level + 2 magnify - 2.  max_level: the largest shown level of a state with a linear combination, the level every top
 * image is decoded at; y_level, c_level: the CODED level of the states the Y plane and the chroma planes are made of.
 * 0 + msg: a gray frame, a band whose shown level would be clamped at 0, a level out of range, or a band without a state
 * at that level (the reference hands out zeros there) */
typedef struct fa_420_plan { unsigned max_level, y_level, c_level; } fa_420_plan;
int fa_420_plan_of(const fa_wfa *w, int color, int magnify, fa_420_plan *plan, char *msg, size_t msg_size);
/* the borders of the 4:2:0 frame at `magnify': the Y phase at shift magnify, the Cb phase at shift magnify - 1, against the
 * size shown (width x height: the coded size).  0 + message as fa_smoothing_borders_magnified */
unsigned fa_smoothing_borders_420(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out,
                                  unsigned cap);
/* ... of a P/B frame of a stream that is walked: the same list without the plan's refusals -- a residual may lack a band,
 * or every linear combination, and decode_image's zeros are then the frame's */
unsigned fa_smoothing_borders_420_residual(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out,
                                           unsigned cap);
void fa_core_release_dev(void *dev, int dev_id);

/* ---------------- stream info (reference codec/wfa.h:65-110 wfa_info_t) ----------- */
typedef struct fa_info {
    char    *basis_name, *title, *comment;
    unsigned max_states, chroma_max_states;
    int      color;
    unsigned width, height, level;
    fa_rpf   rpf, dc_rpf, d_rpf, d_dc_rpf;
    unsigned frames, fps, p_min_level, p_max_level, search_range;
    int      half_pixel, cross_B_search, B_as_past_ref;
    unsigned smoothing;
} fa_info;

/* ---------------- model registries (reference codec/domain-pool.c:188-236, codec/coeff.c:97-131) -----
 * The reference names its domain pools and coefficient models by strings (c_options_t id_domain_pool,
 * id_d_domain_pool, id_rpf_model, id_d_rpf_model; codec/options.c:77-80) and looks them up in two tables;
 * an unknown name gives a warning and the FIRST entry of the table.  Same names, same order, same rule. */
typedef enum fa_pool_kind {
    FA_POOL_ADAPTIVE = 0,       /* "adaptive": quasi-arithmetic model per domain (qac), :259-498 */
    FA_POOL_CONSTANT,           /* "constant": domain list {0}, no model, :504-544 */
    FA_POOL_BASIS,              /* "basis": the adaptive pool over the basis states, :546-560 */
    FA_POOL_UNIFORM,            /* "uniform": every usable state, uniform price, :562-615 */
    FA_POOL_RLE,                /* "rle": the default, :621-879 */
    FA_POOL_RLE_NO_CHROMA       /* "rle-no-chroma": rle whose list is not cut down for the chroma bands, :886-899 */
} fa_pool_kind;
typedef enum fa_coeff_kind { FA_COEFF_ADAPTIVE = 0, FA_COEFF_UNIFORM } fa_coeff_kind;
/* name -> kind; *known = 0 and the table's first entry for a name the table does not hold (the caller warns) */
fa_pool_kind  fa_pool_kind_of(const char *name, int *known);
fa_coeff_kind fa_coeff_kind_of(const char *name, int *known);
const char   *fa_pool_name(fa_pool_kind k);
const char   *fa_coeff_name(fa_coeff_kind k);

/* ---------------- parameters of one frame for the core coder ---------------- */
typedef struct fa_cparams {
    float    price;                       /* 128*64/quality (codec/coder.c:164) */
    unsigned lc_min_level, lc_max_level;  /* after clamping (codec/coder.c:261-281) */
    unsigned images_level, products_level;
    unsigned max_elements;
    unsigned pool_max_states;             /* wi->max_states */
    unsigned chroma_max_states;
    float    chroma_decrease;
    fa_rpf   rpf, dc_rpf, d_rpf, d_dc_rpf;
    int      second_domain_block, check_for_underflow, check_for_overflow, full_search;
    unsigned level;                       /* bintree level of the whole image */
    unsigned limit_states, limit_level;   /* MAXSTATES / MAXLEVEL in force */
    /* prediction (codec/prediction.c) and motion compensation (codec/mwfa.c) */
    int      prediction;                  /* options.prediction: intra (ND) prediction */
    unsigned p_min_level, p_max_level;    /* wi->p_min_level / p_max_level */
    int      delta_domains, normal_domains;
    unsigned search_range;
    int      half_pixel, cross_B_search;
    /* the models (registries above): pool of the normal / of the delta approximation, their coefficient
     * models.  Through fiasco.h only rle / rle / adaptive / adaptive can be had (no setter exists,
     * codec/options.c:77-80); fiasco_amd_c_options_set_models() chooses the others. */
    fa_pool_kind  pool_kind, d_pool_kind;
    fa_coeff_kind coeff_kind, d_coeff_kind;
} fa_cparams;

/* result statistics of one coded band (root range), used for -V 2 style reporting */
typedef struct fa_stats {
    float costs, err, tree_bits, matrix_bits, weights_bits;
} fa_stats;

typedef struct fa_job {
    const fa_image   *image;      /* in  */
    int               frame_type; /* in: FA_I_FRAME / FA_P_FRAME / FA_B_FRAME */
    const fa_image   *past, *future;   /* in: reconstructed reference frames of a P/B frame */
    fa_cparams        cp;         /* in  (lc_min_level may be ratcheted: colour) */
    fa_wfa           *wfa;        /* in: basis states loaded; out: finished automaton */
    fa_stats          stats[3];   /* out */
    int               status;     /* out: 1 ok, 0 failed */
    char              errmsg[160];/* out */
    unsigned          lc_min_level_out; /* out: value of options.lc_min_level after the
                                           frame (colour carry, codec/coder.c:785-797) */
    int               ycol_carry; /* in: wfa->y_column holds what the previous frame of the
                                     stream left there.  The reference keeps ONE wfa_t for a
                                     whole stream and remove_states() (codec/wfalib.c:277-310)
                                     does not clear y_column, so the flags of a colour frame
                                     show through on states of the next frame that are not made
                                     by init_new_state (the three join states).  On return the
                                     array holds this frame's flags for EVERY state id. */
    unsigned          share_key;  /* in: 0 = none, else key + 1: jobs with the same key go to the same device share of
                                     the process whatever their index in the call (fa_share_of) -- the sequence engine
                                     passes the GOP number, so that the frames of a GOP and the decoded reference
                                     frames between them stay on ONE device while other GOPs end */
} fa_job;

/* Which of `shares' device shares (csrc/hip/shares.inc: one per device of the process) takes a job: a pure function of the
 * job's key when it has one, of its index in the call otherwise (round robin).  The search
 * (fa_core_stage) and the decoder (fa_core_decode_frames) both deal with it, so a keyed job is decoded where its
 * successor is searched. */
static inline unsigned fa_share_of(unsigned share_key, unsigned index, unsigned shares)
{
    return shares ? (share_key ? share_key - 1u : index) % shares : 0u;
}

/* THE SEAM.  Encode n independent frames.  Returns number of successful jobs.
 * Staged form: stage() makes the inputs resident where the core computes (HBM for the HIP
 * core), run() encodes every staged frame (may be called repeatedly), unstage() releases.
 * jobs[] must stay alive between stage() and unstage(). */
int   fa_core_encode_frames(unsigned n, fa_job *jobs);
void *fa_core_stage(unsigned n, fa_job *jobs);
int   fa_core_run(void *staged);            /* == submit + finish */
int   fa_core_submit(void *staged);         /* start encoding all staged frames, do not wait */
int   fa_core_finish2(void *staged, int resubmit);   /* finish, and start the next pass as
                                             * early as possible when resubmit != 0 */
int   fa_core_finish(void *staged);         /* wait, bring every frame to completion; the jobs'
                                             * automata are then in host memory and the core is
                                             * free for the next submit */
void  fa_core_unstage(void *staged);
/* Replacing the inputs of a staged batch while a pass runs (a stream of batches):
 *   upload_buffer: host staging memory for `bytes` of int16 planes (pinned for the HIP core),
 *                  valid until the next upload_buffer()/unstage(); NULL = not available
 *   upload_commit: jobs[i].image now describe the new frames, their planes lie inside the
 *                  upload buffer; the core copies them to where it computes WITHOUT waiting
 *                  (overlaps the running pass); the next submit uses them.  1 ok / 0 failed */
int16_t *fa_core_upload_buffer(void *staged, size_t bytes);
int   fa_core_upload_commit(void *staged);
const char *fa_core_name(void);

/* ---------------- bit writer (reference lib/bit-io.c, memory backed) -------------- */
typedef struct fa_bitw {
    unsigned char *buf;
    size_t   cap;
    size_t   bytes;      /* index of current byte + 1 (0 before the first bit) */
    unsigned bitpos;     /* reference semantics: 8 initially, counts down      */
    unsigned long long nbits;
} fa_bitw;
void fa_bw_init(fa_bitw *b);
void fa_bw_free(fa_bitw *b);
void fa_bw_append(fa_bitw *b, const fa_bitw *src);   /* b byte-aligned: what src holds, behind it */
void fa_bw_put_bit(fa_bitw *b, unsigned v);
void fa_bw_put_bits(fa_bitw *b, unsigned v, unsigned n);
void fa_bw_align(fa_bitw *b);
size_t fa_bw_finish(fa_bitw *b);   /* number of bytes the reference would write */
void fa_bw_rice(fa_bitw *b, unsigned value, unsigned k);
void fa_bw_bincode(fa_bitw *b, unsigned value, unsigned maxval);

/* ---------------- bit reader (reference lib/bit-io.c, memory backed, bounds-checked) -------------- */
typedef struct fa_bitr {
    const unsigned char *buf;
    size_t   len;
    size_t   pos;        /* bits consumed */
    int      over;       /* a read went behind the end of the buffer (it gave 0) */
} fa_bitr;
void fa_br_init(fa_bitr *b, const unsigned char *buf, size_t len);
unsigned fa_br_get_bit(fa_bitr *b);
unsigned fa_br_get_bits(fa_bitr *b, unsigned n);
void fa_br_align(fa_bitr *b);
unsigned fa_br_rice(fa_bitr *b, unsigned k);
unsigned fa_br_bincode(fa_bitr *b, unsigned maxval);

/* ---------------- .fco writer (reference output/ directory) ---------------- */
void fa_write_header(const fa_info *wi, fa_bitw *out);
/* returns 1 ok, 0 on the reference's "total != ..." sanity error */
int  fa_write_frame(const fa_wfa *wfa, const fa_info *wi, int frame_type, unsigned number,
                    int prediction, int normal_domains, int delta_domains, fa_bitw *out);
/* ---------------- .fco reader (reference input/ directory; fa_reader.c) ---------------- */
/* The header of the stream in `in' (input/read.c:57-217): *wi filled, the cursor on the first frame.  0 + message */
int  fa_read_header(fa_bitr *in, const char *name, fa_info *wi);
/* The next frame (read_next_wfa, input/read.c:344-451) into an automaton of its own; basis: the automaton
 * fa_load_basis made of the header's basis, copied in front; *number: the display number; flags[3]: prediction,
 * use_normal, use_delta as fa_write_frame takes them.  Everything a decoder follows is validated: NULL + message
 * for a stream that fails */
fa_wfa *fa_read_frame(fa_bitr *in, const fa_info *wi, const fa_wfa *basis, unsigned *number, int flags[3]);

/* ---------------- a stream that was read (include/libfiasco_amd_stream.h; fa_stream.c) ---------------- */
struct fiasco_amd_stream;
const fa_info *fa_stream_info(const struct fiasco_amd_stream *s);
/* The walk of get_next_frame (codec/decoder.c:160-410) over display frames first .. first + count - 1 and every frame
 * they are predicted from, in coding order: frames whose references are decoded go to run() together, as jobs of the
 * decoder with from_stream set (a run of B frames between two P frames: one call where B_as_past_ref is 0, else one
 * frame per call, as each B frame is then the past of the next; a chain of P frames: one frame per
 * call).  display[i]: the display number of jobs[i]; wanted[i]: inside the range asked for -- such a job is smoothed
 * (smoothing resolved: 0 .. 100) and run() attaches its consumer; the others are decoded for reference only.  run()
 * returns after the frames are decoded: a job that succeeded has `out' (an image that holds the device planes where
 * keep_dev is set), a job that failed has its errmsg.  After the walk: result[d - first] holds the image of wanted
 * frame d where keep_images is set (the caller frees it), and errs[d - first] the message of a frame that failed or
 * whose reference did.  mask: NULL, or [count]: 0 = this frame of the range is not wanted.  Returns the number of wanted
 * frames decoded */
typedef void (*fa_stream_run)(void *ctx, unsigned n, fa_dec_job *jobs, const unsigned *display, const uint8_t *wanted);
int fa_stream_walk(const struct fiasco_amd_stream *s, const char *who, unsigned first, unsigned count, const uint8_t *mask, int magnify, int smoothing,
                   int format_420, fa_stream_run run, void *ctx, int keep_images, fa_image **result, char (*errs)[160]);
/* The same walk with its state kept between calls: a cursor.  fa_stream_walk() is one open, one advance over the whole
 * range and one close; a decoder that hands out one display frame per call (fa_decoder.c) advances as it goes, and every
 * coded frame is decoded once per cursor.  open: the range, mask, magnification, smoothing and format of the walk; what
 * each wanted frame is predicted from is worked out here, and the walk's refusals are given here (NULL + message).
 * advance(display, ahead): decodes, in the walk's flights, every frame not yet decoded up to the last coded frame among
 * the wanted display frames display .. display + ahead - 1.  A frame that is a future reference and shown later is
 * decoded then, as a wanted frame: run() gets it once, smoothed for its consumer, and the cursor holds its unsmoothed
 * image for the frames predicted from it.  An image is released as soon as no frame still to come is predicted from it
 * (with keep_images a wanted one stays until it is taken or the cursor is closed); close releases everything.
 * status: 1 decoded, 0 failed (*cause: why, the cursor's string), -1 not decoded yet.  held: images the cursor holds */
typedef struct fa_cursor fa_cursor;
fa_cursor *fa_cursor_open(const struct fiasco_amd_stream *s, const char *who, unsigned first, unsigned count, const uint8_t *mask, int magnify,
                          int smoothing, int format_420, int keep_images);
void      fa_cursor_advance(fa_cursor *c, unsigned display, unsigned ahead, fa_stream_run run, void *ctx);
int       fa_cursor_status(const fa_cursor *c, unsigned display, const char **cause);
fa_image *fa_cursor_take(fa_cursor *c, unsigned display);
unsigned  fa_cursor_held(const fa_cursor *c);
void      fa_cursor_close(fa_cursor *c);
/* the stream in a buffer or a file, as fiasco_amd_stream_open[_file] opens it; name: for the messages */
struct fiasco_amd_stream *fa_stream_open_named(const unsigned char *data, size_t len, const char *name);

/* ---------------- the device side of the decoder objects (csrc/hip/decoder_outlet.inc; fa_decoder.c calls it) ---------- */
/* A fa_stream_run for a cursor: the wanted jobs get the planes outlet of their flight (OcOut::planes) -- the shown planes,
 * smoothed where smoothing applies, Y / Cb / Cr back to back (4:2:0: the chroma planes packed), copied on the flight's
 * stream into a device buffer of their own.  ctx: a fa_outlet, whose planes[display] / device[display] receive the buffer
 * (released with fa_dev_free) */
typedef struct fa_outlet {
    int16_t **planes; int *device;        /* out, by display number */
    size_t    bytes;                      /* of the planes of one frame shown */
    void   *(*take)(void *pool, size_t bytes, int device);     /* a buffer the caller has to spare, or NULL: allocated then */
    void     *pool;
    void    **keep;                       /* the caller's slot for what the share keeps between calls -- its stream, events and
                                           * arena --, made by the first call; released with fa_dev_keep_free */
} fa_outlet;
void  fa_dev_outlet_run(void *ctx, unsigned n, fa_dec_job *jobs, const unsigned *display, const uint8_t *wanted);
void  fa_dev_keep_free(void *keep);
int   fa_dev_available(void);                                  /* 0 + the library's no-device message */
void  fa_dev_free(void *p, int device);
void *fa_dev_upload(const void *host, size_t bytes, int *device);          /* NULL + message */
int   fa_dev_download(void *host, const void *dev, size_t bytes, int device);       /* waits; 0 + message */
/* a staging surface in device memory that grows: *buf of *cap bytes on *device */
int   fa_dev_reserve(void **buf, size_t *cap, size_t bytes, int device);

/* MPEG's code of a vector component, {code, length}, index = component + search range (fa_writer.c) */
extern const unsigned short fa_mv_code[33][2];

/* stable (count desc, state asc) top-n hits, reference codec/wfalib.c:182-231 */
int16_t *fa_compute_hits(unsigned from, unsigned to, unsigned n, const fa_wfa *wfa);

/* ---------------- sequences: frames in coding order, GOPs side by side (fa_sequence.c) ----- */
typedef struct fa_seq fa_seq;
fa_seq *fa_seq_open(const fa_options *op, float quality, unsigned nframes, const unsigned char *const *bufs,
                    const size_t *lens, char const *const *names, unsigned rank, unsigned world);
/* 1 if `pattern' over nframes frames codes a P or B frame one of whose reference frames is missing (`ibbi': an I frame
 * as the future reference of a run of B frames drops the past reference); 0 if not, or if the pattern is not valid */
int fa_seq_pattern_lacks_reference(unsigned nframes, const char *pattern, int B_as_past_ref);
/* the same for frames that are images already (display order; no host planes needed: fa_image.src_dev): the sequence
 * takes images[] and its entries over, also when it refuses them.  release(ctx) runs when the sequence goes -- whoever
 * made the images gives back what their planes lie in (the host C names no core function) */
fa_seq *fa_seq_open_images(const fa_options *op, float quality, unsigned nframes, fa_image **images,
                           unsigned rank, unsigned world);
void    fa_seq_on_free(fa_seq *s, void (*release)(void *ctx), void *ctx);
/* where the searches deliver every reconstructed frame on the device (fa_dec_job's consumer fields): targets, an array
 * of nframes structures of target_size bytes in display order which only the core reads, or NULL; sse, maxdiff
 * [nframes][3] and written [nframes] on the host, or NULL; all borrowed.  Everything NULL: no outputs */
void    fa_seq_set_outputs(fa_seq *s, const void *targets, size_t target_size, unsigned long long *sse, unsigned *maxdiff,
                           unsigned char *written, void *stream);
unsigned fa_seq_nframes(const fa_seq *s);
void    fa_seq_size(const fa_seq *s, unsigned *width, unsigned *height, int *color);
/* the handle of the C ABI around a sequence (takes s over; options == NULL: the defaults, made here) */
fiasco_amd_seq_t *fa_seq_handle(fa_seq *s, fiasco_c_options_t *defaults);
fa_seq *fa_seq_of_handle(const fiasco_amd_seq_t *q);
unsigned fa_seq_display_of(const fa_seq *s, unsigned k);      /* display number of coded frame k */
fa_image *fa_seq_image(const fa_seq *s, unsigned display);    /* fa_seq_open_images: the frame; else NULL */
void    fa_seq_free(fa_seq *s);
int     fa_seq_search(fa_seq *s, const unsigned *carry_in, const uint8_t *todo);
int     fa_seq_probe(fa_seq *s, unsigned *level);
int     fa_seq_encode_all(fa_seq *s, fa_bitw *out,
                          void (*report)(const fa_wfa *, const fa_stats *, const fa_info *));
unsigned fa_seq_gops(const fa_seq *s);
unsigned fa_seq_frames(const fa_seq *s);
unsigned fa_seq_ycol_size(const fa_seq *s);
unsigned fa_seq_initial_level(const fa_seq *s);
unsigned fa_seq_gop_of(const fa_seq *s, unsigned k);
int      fa_seq_is_mine(const fa_seq *s, unsigned gop);
void     fa_seq_gop_result(const fa_seq *s, unsigned gop, unsigned *carry_out, int *failed);
const char *fa_seq_gop_error(const fa_seq *s, unsigned gop);
const fa_stats *fa_seq_stats(const fa_seq *s, unsigned k);
const fa_info *fa_seq_info(const fa_seq *s);
const uint8_t *fa_seq_ycol_raw(const fa_seq *s, unsigned k);
void     fa_seq_ycol_resolve(uint8_t *chain, const uint8_t *raw, unsigned n);
int      fa_seq_write(fa_seq *s, unsigned k, const uint8_t *ycol, fa_bitw *out);

/* ---------------- frame driver pieces shared by fiasco_coder and the batch API ----- */
struct fiasco_amd_batch {
    unsigned   n;
    fa_job    *jobs;
    fa_image **ims;
    fa_image **prev_ims;      /* frames of the pass before the last upload: a pass that was
                               * submitted with them may still be in flight */
    fa_info   *infos;
    int        normal_domains, delta_domains, prediction;
    void      *staged;        /* core handle: inputs resident where the core computes */
};
/* a finished job as a job of the decoder, at magnification `magnify' (fa_batch_decode.c): the one place that fills it.
 * A job that is not a finished intra frame gives skip = 1 and nothing else */
void fa_dec_job_of(const fa_job *job, int magnify, fa_dec_job *d);
/* the job of one still: the automaton with the initial basis loaded (1 ok / 0 + message) */
int fa_prepare_job(fa_job *job, const fa_image *im, const fa_cparams *cp, const char *basis);
unsigned fa_image_level(unsigned width, unsigned height);      /* codec/coder.c:247-255 */
int fa_setup_params(const fa_options *op, float quality, unsigned width, unsigned height,
                    int color, unsigned frames, fa_info *wi, fa_cparams *cp);
void fa_info_free(fa_info *wi);
void fa_limits(unsigned *max_states, unsigned *max_level);

/* ---------------- a renderer (include/libfiasco_amd_render.h; fa_render.c makes it, hip/render.inc reads it) ----- */
struct fiasco_amd_renderer {
    unsigned bpp;             /* 16, 24 or 32 */
    unsigned doubled;         /* 1: every pixel twice in both directions */
    unsigned rgb;             /* 24 bpp: 1 = R, G, B in memory order (red_mask > green_mask), 0 = B, G, R */
    unsigned r_drop, g_drop, b_drop;      /* 8 - bits set in the mask */
    unsigned r_up, g_up, b_up;            /* zero bits below the mask; b_up is kept and NOT applied (the reference's blue) */
};
enum { FA_RENDER_MAX_SIDE = 16384 };      /* of the frame rendered */

#ifdef __cplusplus
}
#endif
#endif
