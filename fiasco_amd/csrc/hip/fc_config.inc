/*
 *  fc_config.inc -- the build configuration of the frame kernel: the geometry of each build
 *  (FC_VARIANT_WIDE, FC_VARIANT_BIG, FC_HM, FC_GM, FC_SPEC: csrc/Makefile), B, FC_KREG and the
 *  per-build kernel and launch symbol names; the FC_SPEC, FC_D5T, FC_IPT and FC_PRIO_ROTATE defaults;
 *  constants; the operation (OP_*) and phase (PH_*) enums; FC_DUP and FC_DEPTH.
 *
 *  Reference: no code of its own; the constants and phases are those of the partition search,
 *  codec/subdivide.c:60-502.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

/* FC_VARIANT_WIDE: FC_WIDE_B (512, or 1024 for the default geometry: csrc/Makefile) threads per
 * frame instead of 256 -- for launches with no more frames than CUs and for frames with more
 * states than 12 x 256 (4K): more lanes per frame, 9216 states in the register slots, one
 * workgroup per CU */
#ifndef FC_VARIANT_WIDE
#define FC_VARIANT_WIDE 0
#endif
#if FC_VARIANT_WIDE
#ifndef FC_WIDE_B
#define FC_WIDE_B 512
#endif
#define B       FC_WIDE_B
#if defined(FC_VARIANT_BIG) && FC_VARIANT_BIG
#define FC_KREG 12               /* 6144 states with 4 orthogonal vectors each in registers */
#elif !defined(FC_KREG)
#define FC_KREG (9216 / FC_WIDE_B)
#endif
#else
#define B       FC_BLOCK
#define FC_KREG 12
#endif
/* Two geometries among the nine builds of frame_coder.hip (csrc/Makefile): the default one for the CLI's
 * -z 0 geometry (block levels 6..10, <= 3 vectors: 4 frames per CU) and FC_VARIANT_BIG for everything else the
 * device supports (block levels 4..12, <= 5 vectors, second-domain retry: 2 frames per CU). */
#ifndef FC_VARIANT_BIG
#define FC_VARIANT_BIG 0
#endif
#if FC_HM && !(FC_VARIANT_BIG && FC_VARIANT_WIDE)
#error "FC_HM is a variant of the 512-thread big build"
#endif
#if FC_GM && !FC_HM
#error "FC_GM is a variant of the FC_HM build"
#endif
#if FC_VARIANT_BIG
#if FC_GM
#define FC_KERNEL    fiasco_frame_kernel_big_gm
#define FC_LAUNCH    fc_launch_big_gm
#define FC_OCCUPANCY fc_occupancy_big_gm
#elif FC_HM
#define FC_KERNEL    fiasco_frame_kernel_big_hm
#define FC_LAUNCH    fc_launch_big_hm
#define FC_OCCUPANCY fc_occupancy_big_hm
#elif FC_VARIANT_WIDE
#define FC_KERNEL    fiasco_frame_kernel_big_wide
#define FC_LAUNCH    fc_launch_big_wide
#define FC_OCCUPANCY fc_occupancy_big_wide
#else
#define FC_KERNEL    fiasco_frame_kernel_big
#define FC_LAUNCH    fc_launch_big
#define FC_OCCUPANCY fc_occupancy_big
#endif
#define FC_PIXELS    4096        /* 2^lc_max, lc_max <= 12 */
#define FC_NIP       4           /* orthogonal vectors kept per candidate: max_elements - 1 */
#define FC_CLMAX     2048
#define FC_WG_PER_CU (FC_VARIANT_WIDE ? 1 : 2)
#else
#if FC_VARIANT_WIDE
#if defined(FC_SPEC) && FC_SPEC
#define FC_KERNEL    fiasco_frame_kernel_spec_wide
#define FC_LAUNCH    fc_launch_spec_wide
#define FC_OCCUPANCY fc_occupancy_spec_wide
#define FC_SPEC_SLOT_BYTES fc_spec_slot_bytes_wide
#elif defined(FC_GRAM_TRI) && FC_GRAM_TRI
#define FC_KERNEL    fiasco_frame_kernel_wide_tri
#define FC_LAUNCH    fc_launch_wide_tri
#define FC_OCCUPANCY fc_occupancy_wide_tri
#else
#define FC_KERNEL    fiasco_frame_kernel_wide
#define FC_LAUNCH    fc_launch_wide
#define FC_OCCUPANCY fc_occupancy_wide
#endif
#elif defined(FC_SPEC) && FC_SPEC
#define FC_KERNEL    fiasco_frame_kernel_spec
#define FC_LAUNCH    fc_launch_spec
#define FC_OCCUPANCY fc_occupancy_spec
#define FC_SPEC_SLOT_BYTES fc_spec_slot_bytes
#else
#define FC_KERNEL    fiasco_frame_kernel
#define FC_LAUNCH    fc_launch
#define FC_OCCUPANCY fc_occupancy
#endif
#define FC_PIXELS    1024
#define FC_NIP       2
#define FC_CLMAX     768         /* Sh::cl: states of a chroma block with table entries somebody reads */
#ifndef FC_WG_PER_CU
/* workgroups (frames) per CU the kernel is built for: four 256-thread frames = 4 waves per SIMD,
 * i.e. at most 128 VGPRs and 40 KB of LDS per frame */
#define FC_WG_PER_CU (FC_VARIANT_WIDE ? 1 : 4)
#endif
#endif
/* FC_SPEC: block-level speculation (frame_coder.h, FcSpecCtl): a frame is served by several
 * workgroups that share its slab -- the 256-thread default build with the chain / verifier roles.
 * A build of its own so that the code of the launches that fill the chip with frames (one
 * workgroup per frame, no spare workgroup slots to speculate with) stays what it is. */
#ifndef FC_SPEC
#define FC_SPEC 0
#endif
#define SPEC_THR 1.2f          /* FC_SPEC: see SpecLocal.mlc */
/* FC_D5T: the table of level-images_level dots is kept state-major, d5T[state][label][NA / 2] (address a ->
 * label a & 1, column a >> 1), so that the first pass of op_ipis reads four consecutive slots of one term with
 * ONE 16-byte load instead of four 4-byte gathers from four rows.  Same values, same sums.  Not in the big
 * build: it reads d5 rows as matching pursuit numerators.  The levels above the first read their sources the same
 * way where FC_IPT is set (below). */
#define FC_D5T (!FC_VARIANT_BIG)
/* FC_IPT: a state-major copy of the block's <sub-block, state> entries of the levels between images_level and lc_max,
 * one table [P][entries of the level] per level (DevFrame.ipt, ipt_layout.h), beside the slot-major table.  Every level
 * of op_ipis_t above the first then reads the `cnt` slots of a term with ONE load of up to 16 bytes from the domain's
 * row, instead of one 4-byte gather per slot from a line per (slot, label, term).  Same values, same sums; the matching
 * pursuit keeps reading slot-major rows.  Every writer of a slot-major entry that a later level may read also writes
 * the ipt entry (op_ipis_t; op_ipis_sparse never mixes with it inside a block).  Not in the big builds, and not in the
 * speculating ones: their blocks' tables live in ring buffers laid out as [NS][P] + [NA][P] (FcSpecCtl.tab_stride). */
#ifndef FC_IPT
#define FC_IPT (!FC_VARIANT_BIG && !FC_SPEC)
#endif
#if FC_IPT && !FC_D5T
#error "FC_IPT goes with the state-major level-images_level dots (FC_D5T)"
#endif
#if FC_D5T
#define D5_AT(P, NA, a, s) ((unsigned) (s) * (unsigned) (NA) + (unsigned) ((a) & 1) * ((unsigned) (NA) >> 1) + ((unsigned) (a) >> 1))
#else
#define D5_AT(P, NA, a, s) ((unsigned) (a) * (unsigned) (P) + (unsigned) (s))
#endif
/* FC_PRIO_ROTATE: rotating instruction priority of the frames that share a CU (kernel loop); the 256-thread default
 * build, whose launches put four workgroups on a CU */
#define FC_PRIO_ROTATE (!FC_VARIANT_BIG && !FC_VARIANT_WIDE && !FC_SPEC)
#define FC_PRIO_SHIFT 20            /* 2^20 ticks of the 100 MHz wall clock: 10 ms per turn (82 us .. 42 ms measured: 580 .. 589 frames/s) */
#define MAXED   FC_MAXED
/* edges per label a state of this build can have (= max_elements the build accepts): the table
 * ops read and gather exactly that many term slots (+ the tree child), not the format's 5 */
#define FC_MAXE (FC_NIP + 1)
#define NOEDGE  (-1)
#define RANGE_  (-1)
#define MAXCOSTS 1e20f
#define BIGF    3.0e38f
#define MIN_NORM 2e-3f

enum { OP_DONE = 0, OP_INIT_RANGE, OP_APPROX, OP_IPIS_INCR, OP_APPEND, OP_NOP, OP_CHROMA,
       OP_PRED_SETUP, OP_PRED_FINISH, OP_NORMS, OP_MC_SEARCH, OP_SPEC_CKPT };
enum { PH_ENTER = 0, PH_AFTER_INIT, PH_AFTER_LC, PH_CHILD, PH_CHILD2, PH_CHILD_RET, PH_DECIDE,
       PH_AFTER_APPEND, PH_PRED_BEGIN, PH_PRED_RECURSE, PH_PRED_RET, PH_PRED_DONE, PH_PRED_MC2, PH_PRED_GO,
       PH_SPEC_END };
enum { MV_NONE = 0, MV_FORWARD = 1, MV_BACKWARD = 2, MV_INTERPOLATED = 3 };
/* FC_DUP_OP=<op>: developer build that runs one of the idempotent table operations (OP_INIT_RANGE, OP_APPEND,
 * OP_IPIS_INCR: they write a function of what they read, the second run writes the same values) TWICE: the difference
 * of the PMC traffic counters to the plain build is that operation's HBM traffic (tests/gpu_traffic_by_op.sh,
 * profiles/r06_traffic_by_op.txt).  Same streams; the roofline counters of the op count double. */
#ifdef FC_DUP_OP
#define FC_DUP(o, call) do { if ((o) == FC_DUP_OP) { __syncthreads(); call; } } while (0)
#else
#define FC_DUP(o, call) do { } while (0)
#endif
#if FC_VARIANT_BIG
#define FC_DEPTH FC_MAXDEPTH_BIG
#elif FC_VARIANT_WIDE
#define FC_DEPTH FC_MAXDEPTH
#else
#define FC_DEPTH FC_MAXDEPTH_NARROW   /* deeper frames go to the 512-thread build (core_hip.cpp) */
#endif
