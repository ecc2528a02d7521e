/*
 *  enc_policy.inc -- what the launcher decides from numbers alone (included by core_hip.cpp): the memory of state
 *  capacities, the workgroups per frame of the table passes (coop), of block-level speculation and of its append
 *  helpers, with the fiasco_amd_*() entries that let the tests ask.
 */

/* Capacity memory.  The first guess of a frame's state capacity (fa_core_stage) is a formula of the frame size;
 * a frame that needs more is searched again with 1.5 x the capacity -- and so would be every later frame of the
 * same kind: the P frames of a 720p colour sequence with --prediction need 1.5 x what their I frames need, and
 * each was searched twice (BASELINE config 5: 20 launches for 10 frames).  So the process remembers, per kind of
 * frame (size, colour, frame type class, block levels, price), the largest need it has seen, and the guess starts
 * there.  The capacity is memory layout only: streams do not depend on it. */
struct CapHint { unsigned long long key; int needP, needPA; };
static pthread_mutex_t g_hint_mu = PTHREAD_MUTEX_INITIALIZER;
static CapHint g_hints[64];
static unsigned g_hint_n, g_hint_next;
static unsigned long long cap_key(const fa_job *job)
{
    const fa_cparams *cp = &job->cp;
    unsigned pb;
    memcpy(&pb, &cp->price, 4);
    const unsigned v[] = { job->image->width, job->image->height, (unsigned) (job->image->color != 0),
                           (unsigned) (job->frame_type != FA_I_FRAME), (unsigned) (cp->prediction != 0), cp->lc_min_level,
                           cp->lc_max_level, cp->p_min_level, cp->p_max_level, cp->max_elements, pb, cp->limit_states };
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++)
        for (int b = 0; b < 4; b++) { h ^= (v[i] >> (8 * b)) & 0xff; h *= 1099511628211ull; }
    return h ? h : 1;
}
static void cap_hint_get(const fa_job *job, int *needP, int *needPA)
{
    const unsigned long long k = cap_key(job);
    *needP = *needPA = 0;
    pthread_mutex_lock(&g_hint_mu);
    for (unsigned i = 0; i < g_hint_n; i++)
        if (g_hints[i].key == k) { *needP = g_hints[i].needP; *needPA = g_hints[i].needPA; break; }
    pthread_mutex_unlock(&g_hint_mu);
}
static void cap_hint_put(const fa_job *job, int needP, int needPA)
{
    const unsigned long long k = cap_key(job);
    pthread_mutex_lock(&g_hint_mu);
    unsigned i = 0;
    for (; i < g_hint_n; i++) if (g_hints[i].key == k) break;
    if (i == g_hint_n) {
        if (g_hint_n < sizeof g_hints / sizeof g_hints[0]) g_hint_n++;
        else i = g_hint_next++ % (sizeof g_hints / sizeof g_hints[0]);       /* full: round robin */
        g_hints[i].key = k; g_hints[i].needP = g_hints[i].needPA = 0;
    }
    if (needP > g_hints[i].needP) g_hints[i].needP = needP;
    if (needPA > g_hints[i].needPA) g_hints[i].needPA = needPA;
    pthread_mutex_unlock(&g_hint_mu);
}

/* workgroups per frame for the table passes of big frames (frame_coder.h FcCoop): the frames are launched in groups
 * of eight (XCD placement), all workgroups must be resident at one per CU */
static unsigned coop_policy(size_t frames, int cus)
{
    const size_t padded = (frames + 7) / 8 * 8;
    if (padded * 8 <= (size_t) cus) return 8;
    if (padded * 4 <= (size_t) cus) return 4;
    if (padded * 2 <= (size_t) cus) return 2;
    return 1;
}
extern "C" unsigned fiasco_amd_coop_workgroups(unsigned frames, int cus) { return coop_policy(frames, cus); }

static size_t top_blocks(const fa_job *job)
{
    const fa_cparams *cp = &job->cp;
    const unsigned bw = fa_width_of_level(cp->lc_max_level), bh = fa_height_of_level(cp->lc_max_level);
    return (size_t) ((job->image->width + bw - 1) / bw) * ((job->image->height + bh - 1) / bh);
}

/* A launch that leaves workgroup slots of the chip free gives its frames several workgroups each
 * (frame_coder.h, FcSpecCtl).  Which frames: gray intra frames of the default geometry whose state
 * capacity -- with room for the verifiers' id ranges -- still fits the 256-thread build.
 * FIASCO_AMD_SPEC=0 switches it off, FIASCO_AMD_SPEC=<G> asks for G workgroups per frame. */
/* of the G workgroups of a frame: the chain, T table workers, G - 1 - T verifiers */
static int spec_workers(int G)
{
    const long long t = knob_int("FIASCO_AMD_SPEC_T", -1);          /* experiments */
    if (t >= 0 && t < G - 1) return (int) t;
    return G >= 6 ? 2 : G >= 4 ? 1 : 0;
}

/* the blocks of the largest block level in the order the partition search visits them
 * (codec/subdivide.c:277-290: the children of a node, first label first; invisible ranges are skipped, :118-120) */
static void spec_block_list(const DevFrame &F, std::vector<uint16_t> &out)
{
    struct Node { int level, x, y; };
    std::vector<Node> stack;
    stack.push_back(Node{F.level, 0, 0});
    out.clear();
    while (!stack.empty()) {
        const Node n = stack.back();
        stack.pop_back();
        if (n.x >= F.width || n.y >= F.height) continue;
        if (n.level == F.lc_max) { out.push_back((uint16_t) n.x); out.push_back((uint16_t) n.y); continue; }
        if (n.level < F.lc_max) continue;
        const int l1 = n.level - 1;
        const int w1 = 1 << (l1 >> 1), h1 = 1 << ((l1 + 1) >> 1);
        /* second child first onto the stack: the first is visited first */
        if (n.level & 1) { stack.push_back(Node{l1, n.x, n.y + h1}); stack.push_back(Node{l1, n.x, n.y}); }
        else             { stack.push_back(Node{l1, n.x + w1, n.y}); stack.push_back(Node{l1, n.x, n.y}); }
    }
}

/* Append helpers per frame (frame_coder.h FcSpecCtl.app_*): further workgroups of a speculating frame that build their
 * shares of every Gram row the chain appends.  For the 1024-thread speculating build (frames beyond 3072 states: 4K),
 * whose launches give a frame a CU per workgroup and leave the rest of the chip empty -- BASELINE config 4 as written
 * puts 8 frames on a GPU: 8 x 8 workgroups on 256 CUs -- and whose rows are long (up to 10 passes of the 1024 lanes).
 * Three where the chip has CUs left for them; fewer than 2 are not worth the hand-off.  A function of its arguments
 * alone (fiasco_amd_spec_append_helpers); FIASCO_AMD_SPEC_APP=<H> (tests, experiments) asks for H at the launch
 * (spec_helpers). */
static size_t spec_app_room(size_t frames, int cus, int G, int occ)
{
    if (occ < 1) occ = 1;
    const size_t room = (size_t) cus * (size_t) occ / frames;       /* workgroups per frame that can be resident */
    return room > (size_t) G ? room - (size_t) G : 0;
}
static int spec_app_policy(size_t frames, int cus, int G, bool wide_build, int occ)
{
    if (!frames || G < 2 || cus < 1) return 0;
    size_t H = spec_app_room(frames, cus, G, occ);
    if (!wide_build) {
        /* the 256-thread build (rows of up to 3072 entries, 12 passes of the lanes): three helpers while the launch
         * stays below 1.5 workgroups per CU -- 1080p: 1 frame 0.367 -> 0.343 s, 16 frames 39.4 -> 42.7, 32 frames 75 -> 80
         * frames/s; 64 and 128 frames (CUs shared by three and more workgroups): nothing, not given */
        return H >= 3 && 2 * frames * ((size_t) G + 3) <= 3 * (size_t) cus ? 3 : 0;
    }
    /* measured (8 x 4K, round 6): 2, 3, 5 and 7 helpers give the same 1.58 .. 1.62 s against 1.87 without -- the hand-off
     * (two releases, two acquires per row) is what a dealt row costs, not the shares; 16 frames 8.5 -> 9.6 frames/s with 3
     * (helpers are light: they may use the half of the chip the frames' own workgroups leave alone, spec_policy) */
    if (H > 3) H = 3;
    return H >= 2 ? (int) H : 0;
}
extern "C" int fiasco_amd_spec_append_helpers(unsigned frames, int cus, int G, int wide_build)
{
    return spec_app_policy(frames, cus, G, wide_build != 0, wide_build ? 1 : 4);      /* the builds' workgroups per CU */
}

/* workgroups per frame of a launch (0: one, no speculation): a function of its arguments alone
 * (fiasco_amd_spec_workgroups, include/libfiasco_amd_hip.h) */
static int spec_policy(size_t frames, int cus, bool big_frames, bool narrow_only, int occ)
{
    if (!frames || cus < 1) return 0;
    /* a CU per workgroup while the frames leave that many, at most FC_SPEC_MAXG; at least two verifiers per chain (one
     * keeps it waiting: slower than no speculation at all) */
    size_t G = (size_t) cus / frames;
    if (G > FC_SPEC_MAXG) G = FC_SPEC_MAXG;
    /* The 256-thread build shares CUs (four workgroups each): as many workgroups per frame as are resident, but not
     * more than five once the launch passes 2.5 workgroups per CU.  Round 6 (hand-offs with one releasing lane;
     * tests/gpu_spec_policy_sweep.sh, 1080p frames/s by workgroups per frame):
     *   frames      3      4      5      6      8     one workgroup each
     *     48       61     76     99     98    104      39
     *     64       81    101    128    127    132      52
     *     96      114    144    186    181    177      78
     *    128      148    189    228    231    203     103
     *    192      195    250    299      (5 is what fits)  154
     *    256      245    275      (4 is what fits)         206
     * (until round 5, when every lane fenced at every hand-off: 5 / 4 / 3 for 64 / 96 / 256 frames -- 113, 132, 213.) */
    if (narrow_only && !big_frames && occ >= 2) {
        G = (size_t) cus * (size_t) occ / frames;
        if (G > FC_SPEC_MAXG) G = FC_SPEC_MAXG;
        if (G > 5 && 2 * frames * G > 5 * (size_t) cus) {
            G = 5 * (size_t) cus / (2 * frames);
            if (G < 5) G = 5;
        }
    }
    /* (Until round 5 4K frames were kept to half the CUs -- 32 frames: 7.2 frames/s with 8 workgroups each, 9.1 with 4:
     * every lane of every workgroup fenced at each hand-off and the L2 write-backs slowed everybody down.  With one
     * releasing lane per hand-off, round 6: 32 frames 10.6 with 4, 15.2 with 6, 15.4 with 8; 24 frames 9.4 -> 13.4.) */
    return G >= 3 ? (int) G : 0;
}

static int spec_groups(size_t frames, int cus, bool big_frames, bool narrow_only)
{
    const char *e = fa_knob("FIASCO_AMD_SPEC");
    if (e && atoi(e) <= 1) return 0;
    if (fa_knob("FIASCO_AMD_TRACE") || fa_knob("FIASCO_AMD_NO_WIDE") || fa_knob("FIASCO_AMD_FORCE_TRI")) return 0;
    int occ = fc_occupancy_spec();
    if (occ < 1) occ = 1;
    if (!frames) return 0;
    if (e) {                                  /* as asked, if the chip holds that many workgroups at once */
        size_t G = (size_t) cus * (size_t) occ / frames;
        if ((size_t) atoi(e) < G) G = (size_t) atoi(e);
        if (G > FC_SPEC_MAXG) G = FC_SPEC_MAXG;
        return G >= 2 ? (int) G : 0;
    }
    return spec_policy(frames, cus, big_frames, narrow_only, occ);
}

extern "C" int fiasco_amd_spec_workgroups(unsigned frames, int cus, int big_frames, int narrow_only, int occupancy)
{
    return spec_policy(frames, cus, big_frames != 0, narrow_only != 0, occupancy);
}
