/*
 *  ipt_layout.h -- where the state-major copy of a block's <sub-block, state> entries keeps them
 *  (DevFrame.ipt, FC_IPT builds): the sources of the level recursion op_ipis_t (fc_tables.inc).
 *
 *  NA = 2^(lc_max - images_level) floats per state in all, as one table PER LEVEL: level lv (images_level < lv <
 *  lc_max) has n = 2^(lc_max - lv) entries per state and is the table [P][n] that starts (NA - 2 n) * P floats into
 *  the buffer -- level images_level + 1 first, the last 2 P floats are padding.  Inside the row of a state the
 *  entries are split by parity as D5_AT splits the level-images_level dots: address a -> label a & 1, column a >> 1.
 *  The sources of `cnt` consecutive slots of level lv + 1 under one label are then `cnt` consecutive floats.  Level
 *  lc_max is never a source and has no table.  Default geometry (NA = 32): level 6 [P][16] at 0, level 7 [P][8] at
 *  16 P, level 8 [P][4] at 24 P, level 9 [P][2] at 28 P.
 *
 *  One table per level, not one row of NA floats per state with the levels side by side: a pass of the recursion
 *  reads ONE level of every domain, and with the levels side by side it pulls the whole 128-byte line of a state in for
 *  the 64, 32, 16 or 8 bytes it wants (measured: 8.6 % slower than slot-major gathers, where this form is 1.4 %
 *  faster; LABNOTES).
 *
 *  Plain C++ without a dependency: the frame kernel includes it, and so does the host-side check of the
 *  layout (tests/ipt_layout_check.cpp).
 */
#ifndef FIASCO_IPT_LAYOUT_H
#define FIASCO_IPT_LAYOUT_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IPT_FN __host__ __device__ inline
#else
#define IPT_FN inline
#endif

/* entries per state of level lv */
IPT_FN unsigned ipt_n(int lc_max, int lv) { return 1u << (lc_max - lv); }
/* first float of state s in the table of the level with n entries per state (P: capacity for states with tables) */
IPT_FN unsigned ipt_row(unsigned P, unsigned NA, unsigned n, unsigned s) { return (NA - 2u * n) * P + s * n; }
/* entry of address a inside a state's row of the level with n entries */
IPT_FN unsigned ipt_col(unsigned n, unsigned a) { return (a & 1u) * (n >> 1) + (a >> 1); }
/* source of the slot of address a, label l, of the level with n entries, inside the DOMAIN's row of the level below
 * (2 n entries): the entry of address 2 a + l */
IPT_FN unsigned ipt_src_col(unsigned n, unsigned l, unsigned a) { return l * n + a; }
/* floats per load and term of a level with `cnt` slots in the call's subtree (groups of at most four slots): 4, 2 or 1 */
IPT_FN unsigned ipt_width(unsigned cnt) { return cnt >= 4u ? 4u : cnt; }

/*
 *  Work items of the level recursion: a level with `cnt` slots in the call's subtree gives every state
 *  G = cnt >= 8 ? cnt / 4 : 1 neighbouring lanes, one per group of four slots (4 lanes at the first level of a whole
 *  block of the default geometry, 2 at the second, 1 above).  Item i = tid + k B serves state `from` + i / G and the
 *  slots j0 .. j0 + 3 of the subtree, j0 = 4 (i % G).  G is a power of two that divides the wave and the workgroup: the
 *  lanes of a state are an aligned group of one wave, i % G is the same in every round k, and the G loads of a term are
 *  G neighbouring 16-byte pieces of the domain's row in one instruction.  Every lane stores its own results, as pairs of
 *  equal parity (whole rows through an exchange inside the quad measured slower: LABNOTES, experiments/ipis_items).
 */
/* log2 of the lanes per state (cnt is a power of two) */
IPT_FN unsigned ipis_lanes_log2(unsigned cnt) { return cnt >= 8u ? (unsigned) __builtin_ctz(cnt) - 2u : 0u; }
IPT_FN unsigned ipis_lanes(unsigned cnt) { return 1u << ipis_lanes_log2(cnt); }
/* state of item i, counted from the call's first state; first slot of its group, counted from the subtree's first */
IPT_FN unsigned ipis_item_state(unsigned i, unsigned lgG) { return i >> lgG; }
IPT_FN unsigned ipis_item_j0(unsigned i, unsigned lgG) { return 4u * (i & ((1u << lgG) - 1u)); }

#endif
