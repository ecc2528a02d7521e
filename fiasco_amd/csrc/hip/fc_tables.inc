/*
 *  fc_tables.inc -- the parallel table operations: <sub-block, state> inner products (op_ipis,
 *  op_d5); several workgroups for the table passes of one frame (FcCoop, coop_*); the chroma-need
 *  closure with op_d5_sparse and op_ipis_sparse; op_init_range.
 *
 *  Reference: inner-product tables codec/ip.c:46-323; init_range codec/subdivide.c:504-541,612-644.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */
#include "ipt_layout.h"               /* where the state-major copy of the recursion's sources keeps an entry (FC_IPT) */

/* ------------------------------------------------------------------ parallel ops */

/* <sub-block, state> tables in use: the block's, or -- big build, while the residual of a
 * predicted range is searched (codec/prediction.c:302-309,443-450) -- the second set */
#if FC_VARIANT_BIG
#define ACT_IPIS(F, sh) ((sh).par.ipis)
#define ACT_D5(F, sh)   ((sh).par.d5)
#define ACT_D4(F, sh)   ((sh).par.d4)
#elif FC_SPEC               /* the block's tables live in one buffer of the frame's ring, or in the workgroup's own */
#define ACT_IPIS(F, sh) ((sh).par.ipis)
#define ACT_D5(F, sh)   ((sh).par.d5)
#define ACT_D4(F, sh)   ((F).d4)
#else
#define ACT_IPIS(F, sh) ((F).ipis)
#define ACT_D5(F, sh)   ((F).d5)
#define ACT_D4(F, sh)   ((F).d4)
#endif

/* states that can own tables: chroma states are all auxiliary (codec/subdivide.c:433-436) */
__device__ __forceinline__ int table_states(const Sh &sh) { return sh.band ? sh.ystates : sh.states; }

/* the automaton arrays of a frame behind uniform global pointers */
struct AutoTabs {
    GLOBAL_AS const int16_t *tree, *into;
    GLOBAL_AS const float   *weight;
    GLOBAL_AS const uint8_t *domain_type;
    int PA;
};

__device__ __forceinline__ void auto_tabs(const DevFrame &F, AutoTabs &t)
{
    t.tree = uniform_ptr((const int16_t *) F.tree); t.into = uniform_ptr((const int16_t *) F.into);
    t.weight = uniform_ptr((const float *) F.weight);
    t.domain_type = uniform_ptr((const uint8_t *) F.domain_type);
    t.PA = __builtin_amdgcn_readfirstlane(F.PA);
}

/* the automaton rows of one state as they come out of memory: all edge slots are read
 * unconditionally (independent, coalesced loads; what lies behind the terminator is ignored) */
template <int E> struct EdgeRowsT {
    int   tree[2], rd[2][E];
    float rw[2][E];
    int   dt;
};
typedef EdgeRowsT<FC_MAXE> EdgeRows;

template <int E> __device__ __forceinline__ void load_edge_rows(const AutoTabs &T, int s, EdgeRowsT<E> &r)
{
    unsigned us = (unsigned) s;
    /* opaque to loop strength reduction: otherwise every array gets its own 64-bit pointer
     * induction variable in VGPRs (46 registers) instead of scalar base + this one offset */
    asm volatile("" : "+v"(us));
    r.dt = ldg(T.domain_type, us);
#pragma unroll
    for (int l = 0; l < 2; l++) {
        /* one scalar base per array, the row offset goes into the lane offset */
        r.tree[l] = ldg(T.tree, us + (unsigned) (l * T.PA));
#pragma unroll
        for (int e = 0; e < E; e++) {
            r.rd[l][e] = ldg(T.into, us + (unsigned) ((l * 6 + e) * T.PA));
            r.rw[l][e] = ldg(T.weight, us + (unsigned) ((l * 6 + e) * T.PA));
        }
    }
}

#if FC_IPT
/* term list of a state for the item loop of op_ipis_t: per label the tree child (weight 1, added plain) and
 * the edges in stored order.  Fixed-trip, predicated loops so that all loads of a group of slots are in
 * flight together (the chain is latency bound).  msk: bit 0 the child, bit e + 1 edge e; a dead term has
 * index 0 and weight 0. */
template <int E> __device__ __forceinline__ void ipis_terms(const EdgeRowsT<E> &cur, int (&idx)[2][E + 1], float (&wt)[2][E + 1], unsigned (&msk)[2])
{
#pragma unroll
    for (int l = 0; l < 2; l++) {
        int k = cur.tree[l];
        msk[l] = k != RANGE_ ? 1u : 0u;
        idx[l][0] = k != RANGE_ ? k : 0;
        wt[l][0] = 1.0f;
        bool live = true;
#pragma unroll
        for (int e = 0; e < E; e++) {
            live = live && cur.rd[l][e] != NOEDGE;
            idx[l][e + 1] = live ? cur.rd[l][e] : 0;
            wt[l][e + 1] = live ? cur.rw[l][e] : 0.0f;
            msk[l] |= live ? (2u << e) : 0u;
        }
    }
}
#endif

/* <sub-block, state> tables for states [from, states) and the heap subtree under `image`
 * (codec/ip.c:72-154).  Per slot the additions run label 0 {child, edges}, label 1 {...}
 * onto zero, which is the reference's accumulation order onto its zeroed slots.
 * FC_IPT: the levels above the first read their sources from the state-major copy DevFrame.ipt, and every level
 * below lc_max writes its results there as well as slot-major (fc_config.inc, ipt_layout.h). */
/* E: edge slots per label read and summed (the build's E; 3 in the big build when neither the options nor
 * the basis allow more: dead slots still cost a gather per slot and state) */
template <int E> __device__ __noinline__ void op_ipis_t(const DevFrame &__restrict__ F, Sh &__restrict__ sh, int image, int address, int level, int from, int lv_first)
{
#if FC_IPT
    /* wave-uniform, so that the level, its slot count and the choice of the source table stay in scalar registers */
    const int tid = threadIdx.x, il = __builtin_amdgcn_readfirstlane(F.images_level);
#else
    const int tid = threadIdx.x, il = F.images_level;
#endif
    const int P = __builtin_amdgcn_readfirstlane(F.P), states = __builtin_amdgcn_readfirstlane(table_states(sh));
    image = __builtin_amdgcn_readfirstlane(image); address = __builtin_amdgcn_readfirstlane(address);
    level = __builtin_amdgcn_readfirstlane(level); from = __builtin_amdgcn_readfirstlane(from);
    GLOBAL_AS float *const ipis = uniform_ptr(ACT_IPIS(F, sh));
    GLOBAL_AS const float *const d5 = uniform_ptr((const float *) ACT_D5(F, sh));
#if FC_IPT
    /* the state-major copy of the entries below level lc_max (ipt_layout.h): what the levels above the first read,
     * and where every level below lc_max leaves its results beside the slot-major ones */
    GLOBAL_AS float *const ipt = uniform_ptr(F.ipt);
    const int lc_max = __builtin_amdgcn_readfirstlane(F.lc_max);
#endif
    AutoTabs T;
    auto_tabs(F, T);
    lv_first = __builtin_amdgcn_readfirstlane(lv_first);
    for (int lv = lv_first > il + 1 ? lv_first : il + 1; lv <= level; lv++) {
        int delta = level - lv;
        int cnt = 1 << delta;
        int slot0 = ((image + 1) << delta) - 1;
        int adr0 = address << delta;
#if FC_D5T
        const bool first = lv == il + 1;
        const unsigned NAu = (unsigned) __builtin_amdgcn_readfirstlane(F.NA), NAh = NAu >> 1;
#if FC_IPT
        /* State-major sources at every level: the cnt slots of a term and label are cnt consecutive floats of the
         * domain's row -- of d5 at the first level (NA floats per state), of the ipt table of the level below above
         * it (2 n_lv floats per state) -- from float lb[label] + adr0 of the row on.  cnt is a power of two and adr0
         * a multiple of it, and so are the rows and their halves wherever they hold cnt or more entries: every
         * load is aligned to its width (tests/ipt_layout_check.cpp walks them all). */
        const unsigned n_lv = ipt_n(lc_max, lv);
        GLOBAL_AS const float *src0 = first ? d5 : (GLOBAL_AS const float *) ipt;
        const unsigned Pu = (unsigned) P, rs = first ? NAu : 2u * n_lv;
        const unsigned lb[2] = { first ? 0u : ipt_row(Pu, NAu, 2u * n_lv, 0u) + ipt_src_col(n_lv, 0u, 0u),
                                 first ? NAh : ipt_row(Pu, NAu, 2u * n_lv, 0u) + ipt_src_col(n_lv, 1u, 0u) };
#else
        const bool vec4 = first && cnt >= 4 && (NAh & 3u) == 0;          /* adr0 is a multiple of cnt */
        GLOBAL_AS const float *src0 = first ? d5 : ipis + (size_t) (slot0 * 2 + 1) * P;
#endif
#else
        GLOBAL_AS const float *src0 = (lv == il + 1) ? d5 + (size_t) (adr0 * 2) * P
                                                     : ipis + (size_t) (slot0 * 2 + 1) * P;
#endif
        int s = from + tid;
#if FC_VARIANT_BIG
        if (F.bx) {                        /* basis states with their terms in DevFrame.bx (see bx_view) */
            const BxView V = bx_view(F);
            for (int i = tid; i < V.nb * cnt; i += B) {
                const int bs = i / cnt, j = i - bs * cnt;
                if (bs < from || !V.dtype[bs]) continue;
                float acc = 0;
                for (int l = 0; l < 2; l++) {
                    int dom;
                    for (int e = (bs * 2 + l) * 6; (dom = V.into[e]) != NOEDGE; e++)
                        acc += V.w[e] * ldg(src0, (unsigned) dom + (unsigned) ((j * 2 + l) * P));
                }
                stg(ipis, (unsigned) bs + (unsigned) ((slot0 + j) * P), acc);
            }
            if (from < V.nb) s = V.nb + tid;
        }
#endif
#if FC_IPT
        /* Work items, not states (ipt_layout.h): G = cnt / 4 neighbouring lanes serve one state where the level has 8 or
         * more slots in the subtree, one group of four slots each -- the loads of a term by the lanes of a state are
         * neighbouring 16-byte pieces of one row in ONE instruction, and a lane has one round of loads per level
         * instead of cnt / 4 dependent ones.  G divides the wave and B: the lanes of a state are neighbours in one wave
         * with the same state in every round (tests/ipis_items_check.cpp walks them all). */
        const unsigned lgG = ipis_lanes_log2((unsigned) cnt), j0 = ipis_item_j0((unsigned) tid, lgG);
        const int sB = B >> lgG;
        s = from + (int) ipis_item_state((unsigned) tid, lgG);
        /* the rows of the NEXT item of this lane are requested before the loads of the current one are waited for */
        EdgeRowsT<E> nx;
        if (s < states) load_edge_rows(T, s, nx);
        for (; s < states; s += sB) {
            const EdgeRowsT<E> cur = nx;
            if (s + sB < states) load_edge_rows(T, s + sB, nx);
            const bool tabled = cur.dt && !DEAD(sh, s);
            if (!tabled) continue;
            int   idx[2][E + 1];
            float wt[2][E + 1];
            unsigned msk[2];
            ipis_terms<E>(cur, idx, wt, msk);
            float v[4][2][E + 1];
            /* UNCONDITIONAL loads (a dead term reads the same columns of row 0, which lie inside the table
             * whatever they hold): a conditional load becomes a branch with its own s_waitcnt and the loads
             * would run one after the other instead of all in flight.  ONE load per term and label brings
             * all slots of the group: 16 bytes for four, 8 for the two slots of the level below the call's,
             * 4 for the call's own slot -- no slot is read that the group does not have. */
            /* one scalar base and one 32-bit byte offset per term, whatever the width (ldg's addressing) */
            unsigned ob[2][E + 1];
#pragma unroll
            for (int l = 0; l < 2; l++)
#pragma unroll
                for (int i = 0; i <= E; i++) ob[l][i] = ((unsigned) idx[l][i] * rs + lb[l] + (unsigned) adr0 + j0) * 4u;
            typedef float f4 __attribute__((ext_vector_type(4)));
            typedef float f2 __attribute__((ext_vector_type(2)));
            if (cnt >= 4) {
#pragma unroll
                for (int l = 0; l < 2; l++)
#pragma unroll
                    for (int i = 0; i <= E; i++) {
                        const f4 q = *(GLOBAL_AS const f4 *) ((GLOBAL_AS const char *) src0 + ob[l][i]);
                        v[0][l][i] = q.x; v[1][l][i] = q.y; v[2][l][i] = q.z; v[3][l][i] = q.w;
                    }
            } else if (cnt == 2) {
#pragma unroll
                for (int l = 0; l < 2; l++)
#pragma unroll
                    for (int i = 0; i <= E; i++) {
                        const f2 q = *(GLOBAL_AS const f2 *) ((GLOBAL_AS const char *) src0 + ob[l][i]);
                        v[0][l][i] = q.x; v[1][l][i] = q.y;
                    }
            } else {
#pragma unroll
                for (int l = 0; l < 2; l++)
#pragma unroll
                    for (int i = 0; i <= E; i++)
                        v[0][l][i] = *(GLOBAL_AS const float *) ((GLOBAL_AS const char *) src0 + ob[l][i]);
            }
            float res[4];
            /* slot-major, what the matching pursuit reads: plain 4-byte stores */
            const unsigned os = (unsigned) s + j0 * Pu;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                if (jj >= cnt) break;
                float acc = 0;
#pragma unroll
                for (int l = 0; l < 2; l++) {
                    if (msk[l] & 1u) acc += v[jj][l][0];
#pragma unroll
                    for (int i = 1; i <= E; i++)
                        if ((msk[l] >> i) & 1u) acc += wt[l][i] * v[jj][l][i];
                }
                stg(ipis + (size_t) ((slot0 + jj) * P), os, acc);
                res[jj] = acc;
            }
            /* ... and, below level lc_max, into the state's row of this level's ipt table, for the level above */
            if (lv < lc_max) {
                const unsigned a0 = (unsigned) adr0 + j0, row = ipt_row(Pu, NAu, n_lv, (unsigned) s);
                if (cnt >= 4) {
                    /* the even and the odd addresses of a group of four are two neighbouring columns each */
                    const f2 ev = { res[0], res[2] }, od = { res[1], res[3] };
                    *(GLOBAL_AS f2 *) ((GLOBAL_AS char *) ipt + (row + ipt_col(n_lv, a0)) * 4u) = ev;
                    *(GLOBAL_AS f2 *) ((GLOBAL_AS char *) ipt + (row + ipt_col(n_lv, a0 + 1u)) * 4u) = od;
                } else {
                    stg(ipt, row + ipt_col(n_lv, a0), res[0]);
                    if (cnt == 2) stg(ipt, row + ipt_col(n_lv, a0 + 1u), res[1]);
                }
            }
        }
#else
        /* the rows of the NEXT state of this lane are requested before the gathers of the
         * current one are waited for (one memory round trip per state instead of two) */
        EdgeRowsT<E> nx;
        if (s < states) load_edge_rows(T, s, nx);
        for (; s < states; s += B) {
            const EdgeRowsT<E> cur = nx;
            if (s + B < states) load_edge_rows(T, s + B, nx);
            const bool tabled = cur.dt && !DEAD(sh, s);
            if (!tabled) continue;
            /* term list of the state: per label the tree child (weight 1, added plain) and
             * the edges in stored order.  Fixed-trip, predicated loops so that all gathers
             * of a group of slots are in flight together (the chain is latency bound). */
            int   idx[2][E + 1];
            float wt[2][E + 1];
            unsigned msk[2];
#pragma unroll
            for (int l = 0; l < 2; l++) {
                int k = cur.tree[l];
                msk[l] = k != RANGE_ ? 1u : 0u;
                idx[l][0] = k != RANGE_ ? k : 0;
                wt[l][0] = 1.0f;
                bool live = true;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    live = live && cur.rd[l][e] != NOEDGE;
                    idx[l][e + 1] = live ? cur.rd[l][e] : 0;
                    wt[l][e + 1] = live ? cur.rw[l][e] : 0.0f;
                    msk[l] |= live ? (2u << e) : 0u;
                }
            }
            constexpr int JG = 4;          /* slots per group: 4 x 2 x (E + 1) gathers in flight per lane (8: -5 %) */
            for (int j0 = 0; j0 < cnt; j0 += JG) {
                float v[JG][2][E + 1];
#if FC_D5T
                if (vec4) {
                    typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
                    for (int l = 0; l < 2; l++)
#pragma unroll
                        for (int i = 0; i <= E; i++) {
                            const unsigned o = (unsigned) idx[l][i] * NAu + (unsigned) l * NAh + (unsigned) (adr0 + j0);
                            const f4 q = *(GLOBAL_AS const f4 *) (src0 + o);
                            v[0][l][i] = q.x; v[1][l][i] = q.y; v[2][l][i] = q.z; v[3][l][i] = q.w;
                        }
                } else if (first) {
#pragma unroll
                    for (int jj = 0; jj < JG; jj++)
#pragma unroll
                        for (int l = 0; l < 2; l++)
#pragma unroll
                            for (int i = 0; i <= E; i++) {
                                const int jc = j0 + jj < cnt ? j0 + jj : cnt - 1;
                                v[jj][l][i] = ldg(src0, (unsigned) idx[l][i] * NAu + (unsigned) l * NAh + (unsigned) (adr0 + jc));
                            }
                } else
#endif
#pragma unroll
                for (int jj = 0; jj < JG; jj++)
#pragma unroll
                    for (int l = 0; l < 2; l++)
#pragma unroll
                        for (int i = 0; i <= E; i++) {
                            /* UNCONDITIONAL loads (dead terms read element 0 of the row, slots
                             * past the end re-read the last one): a conditional load becomes a
                             * branch with its own s_waitcnt and the gathers would run one
                             * after the other instead of all in flight */
                            const int jc = j0 + jj < cnt ? j0 + jj : cnt - 1;
                            v[jj][l][i] = ldg(src0, (unsigned) idx[l][i] + (unsigned) ((jc * 2 + l) * P));
                        }
#pragma unroll
                for (int jj = 0; jj < JG; jj++) {
                    if (j0 + jj >= cnt) break;
                    float acc = 0;
#pragma unroll
                    for (int l = 0; l < 2; l++) {
                        if (msk[l] & 1u) acc += v[jj][l][0];
#pragma unroll
                        for (int i = 1; i <= E; i++)
                            if ((msk[l] >> i) & 1u) acc += wt[l][i] * v[jj][l][i];
                    }
                    stg(ipis, (unsigned) s + (unsigned) ((slot0 + j0 + jj) * P), acc);
                }
            }
        }
#endif
        __syncthreads();
    }
}

/* lv_first: the levels below it are in the tables already (a cooperative build, FcCoop) */
__device__ __forceinline__ void op_ipis(const DevFrame &__restrict__ F, Sh &__restrict__ sh, int image, int address, int level, int from,
                                        int lv_first = 0)
{
#if FC_VARIANT_BIG
    if (F.maxe_live <= 3) { op_ipis_t<3>(F, sh, image, address, level, from, lv_first); return; }
#endif
    op_ipis_t<FC_MAXE>(F, sh, image, address, level, from, lv_first);
}

/* level-images_level dots of the current pixel block with state images (codec/ip.c:268-295) */
/* na / n4: number of level-images_level and level-(images_level - 1) sub-blocks of the block in
 * sh.pixels (NA and 2 NA for a whole block; fewer for the residual of a predicted range) */
/* abase / pxoff: the addresses start at abase (level images_level; 2 abase one level below) and their pixels at
 * sh.pixels + pxoff -- one subtree of a block (cooperative build, FcCoop) */
__device__ void op_d5(const DevFrame &__restrict__ F, Sh &__restrict__ sh, int from, int to, int na, int n4, int abase = 0, int pxoff = 0)
{
    const int tid = threadIdx.x, P = __builtin_amdgcn_readfirstlane(F.P);
    /* tables behind scalar bases: global_load / global_store with a 32-bit lane offset (through the generic
     * frame reference of this out-of-line code they would be flat_ instructions) */
    GLOBAL_AS float *const D5 = uniform_ptr(ACT_D5(F, sh));
    GLOBAL_AS const float *const imgT = uniform_ptr((const float *) F.imgT);
    GLOBAL_AS const uint8_t *const dtype = uniform_ptr((const uint8_t *) F.domain_type);
    for (int s = from + tid; s < to; s += B) {
        if (DEAD(sh, s) || !ldg(dtype, (unsigned) s)) continue;
        float v[32];
#pragma unroll
        for (int k = 0; k < 32; k++) v[k] = ldg(imgT, (unsigned) (k * P + s));
        /* two addresses per step: packed fp32 multiply and add (v_pk_mul_f32 / v_pk_add_f32,
         * each half rounded like the scalar op; no fused multiply-add), pixels read in pairs */
        typedef float f2 __attribute__((ext_vector_type(2)));
#if FC_D5T
        const unsigned NAu = (unsigned) __builtin_amdgcn_readfirstlane(F.NA), NAh = NAu >> 1;
        int a = 0;
        if ((NAh & 3u) == 0)
            /* eight addresses per step: the even and the odd ones are four consecutive floats each */
            for (; a + 8 <= na; a += 8) {
                f2 ip[4] = { { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f } };
#pragma unroll
                for (int k = 0; k < 32; k++) {
                    f2 vv = { v[k], v[k] };
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        f2 px = { sh.pixels[(a + 2 * u) * 32 + k], sh.pixels[(a + 2 * u) * 32 + 32 + k] };
                        ip[u] = ip[u] + px * vv;
                    }
                }
                typedef float f4 __attribute__((ext_vector_type(4)));
                const f4 ev = { ip[0].x, ip[1].x, ip[2].x, ip[3].x }, od = { ip[0].y, ip[1].y, ip[2].y, ip[3].y };
                const unsigned o = (unsigned) s * NAu + ((unsigned) a >> 1);
                *(GLOBAL_AS f4 *) (D5 + o) = ev;
                *(GLOBAL_AS f4 *) (D5 + o + NAh) = od;
            }
        for (; a < na; a += 2) {
            f2 ip = { 0.0f, 0.0f };
#pragma unroll
            for (int k = 0; k < 32; k++) {
                f2 px = { sh.pixels[a * 32 + k], sh.pixels[a * 32 + 32 + k] };
                f2 vv = { v[k], v[k] };
                ip = ip + px * vv;
            }
            stg(D5, D5_AT(P, NAu, a, s), ip.x);
            if (a + 1 < na) stg(D5, D5_AT(P, NAu, a + 1, s), ip.y);
        }
#else
        for (int a = 0; a < na; a += 2) {
            f2 ip = { 0.0f, 0.0f };
#pragma unroll
            for (int k = 0; k < 32; k++) {
                f2 px = { sh.pixels[pxoff + a * 32 + k], sh.pixels[pxoff + a * 32 + 32 + k] };
                f2 vv = { v[k], v[k] };
                ip = ip + px * vv;
            }
            stg(D5, (unsigned) ((abase + a) * P + s), ip.x);
            if (a + 1 < na) stg(D5, (unsigned) ((abase + a + 1) * P + s), ip.y);
        }
#endif
#if FC_VARIANT_BIG
        if (F.gl0 < F.images_level) {
            float *const D4 = ACT_D4(F, sh);
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = F.imgT4[(size_t) k * P + s];
            for (int a = 0; a < n4; a++) {
                float ip = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) ip += sh.pixels[pxoff + a * 16 + k] * v[k];
                D4[(size_t) (2 * abase + a) * P + s] = ip;
            }
        }
#endif
    }
}

#if FC_VARIANT_BIG
/* ---- several workgroups for the table passes of one frame (frame_coder.h, FcCoop) ---- */
__device__ __forceinline__ float *coop_pixels(FcCoop *c) { return (float *) ((char *) c + FC_COOP_HDR); }

/* the subtrees member, member + W, ... of depth D below a block of 2^level pixels in sh.pixels: level-5 dots and
 * the level recursion up to the subtree's own level, for the states [from, table_states) */
__device__ void coop_share(const DevFrame &__restrict__ F, Sh &__restrict__ sh, int level, int from, unsigned member, unsigned W, int D)
{
    const int il = F.images_level, sub = level - D, nasub = 1 << (sub - il);
    for (int j = (int) member; j < (1 << D); j += (int) W)
        op_d5(F, sh, from, table_states(sh), nasub, 2 * nasub, j * nasub, j << sub);
    __syncthreads();
    for (int j = (int) member; j < (1 << D); j += (int) W)
        op_ipis(F, sh, (1 << D) - 1 + j, j, sub, from);
}

/* The frame's workgroup: hand the block in sh.pixels to the helpers.  Returns the depth D (the caller goes on
 * with coop_finish and adds the levels above level - D), or 0: the block is built the ordinary way. */
__device__ int coop_publish(DevFrame &__restrict__ F, Sh &__restrict__ sh, int level, int from)
{
    const int tid = threadIdx.x, il = F.images_level;
    const unsigned W = sh.coopW;
    FcCoop *c = F.coop;
    if (W < 2 || !c) return 0;
    const int D = sh.coopD;
    if (level - il < D + sh.coop_minsub) return 0;          /* small subtrees: not worth a hand-off */
    float *gp = coop_pixels(c);
    for (int i = tid; i < (1 << level); i += B) gp[i] = sh.pixels[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        c->level = level; c->from = from; c->to = table_states(sh);
        c->ipis = sh.par.ipis; c->d5 = sh.par.d5; c->d4 = sh.par.d4;
        /* everything the helpers read: the pixels, the descriptor, the rows of the states appended so far */
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        sh.coop_seq++;
        __hip_atomic_store(&c->seq, sh.coop_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return D;
}

/* ... after the caller's own LDS-only work (the norms of the block): the own share, then the helpers' */
__device__ void coop_finish(DevFrame &__restrict__ F, Sh &__restrict__ sh, int level, int from, int D)
{
    const int tid = threadIdx.x;
    const unsigned W = sh.coopW;
    FcCoop *c = F.coop;
    coop_share(F, sh, level, from, 0, W, D);
    __syncthreads();
    if (tid == 0) {
        const unsigned want = sh.coop_seq * (W - 1);
        const unsigned long long t_give_up = wall_clock64() + sh.coop_ticks;
        while (__hip_atomic_load(&c->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
            if (wall_clock64() > t_give_up) { sh.failed = FC_ERR_COOP; break; }
            __builtin_amdgcn_s_sleep(4);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      /* the helpers' rows, not this CU's stale lines */
    }
    __syncthreads();
}

/* workgroups 1 .. W - 1 of a frame: build what the frame's workgroup hands over until it is finished */
__device__ void coop_helper(DevFrame &__restrict__ F, Sh &__restrict__ sh, unsigned member, unsigned W)
{
    const int tid = threadIdx.x;
    FcCoop *c = F.coop;
    unsigned seen = 0;
    if (!c) return;
    for (;;) {
        if (tid == 0) {
            const unsigned long long t_give_up = wall_clock64() + FC_COOP_WAIT_TICKS;
            int go = 0;
            for (;;) {
                if (__hip_atomic_load(&c->quit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { go = -1; break; }
                if (__hip_atomic_load(&c->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seen) { go = 1; break; }
                if (wall_clock64() > t_give_up) { go = -1; break; }
                __builtin_amdgcn_s_sleep(8);
            }
            if (go == 1) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                sh.a0 = c->level; sh.a1 = c->from; sh.a2 = (int) c->depth;
                sh.band = 0; sh.states = c->to; sh.ystates = c->to;
                sh.par.ipis = c->ipis; sh.par.d5 = c->d5; sh.par.d4 = c->d4;
            }
            sh.op = go;
        }
        __syncthreads();
        if (sh.op < 0) return;
        const int level = sh.a0, from = sh.a1, D = sh.a2, sub = level - D;
        const float *gp = coop_pixels(c);
        for (int j = (int) member; j < (1 << D); j += (int) W)
            for (int i = tid; i < (1 << sub); i += B) sh.pixels[(j << sub) + i] = gp[(j << sub) + i];
        __syncthreads();
        coop_share(F, sh, level, from, member, W, D);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(&c->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        seen++;
        __syncthreads();                /* sh.op is rewritten by lane 0 at the top */
    }
}
#endif

#if !FC_SPEC
/* ------------------------------------------------------------------ chroma bands: tables for the states that matter
 *
 * init_range builds the <sub-block, state> entries of a block for EVERY state with tables (codec/subdivide.c:612-644,
 * codec/ip.c:72-154).  In a chroma band nobody appends a state with tables (chroma states are auxiliary,
 * codec/subdivide.c:433-436) and nothing is predicted: the entries are read by the matching pursuit of the block's
 * ranges alone -- for the <= chroma_max states of the chroma list plus the co-located luminance state of the range
 * (rle_generate, codec/domain-pool.c:707-735) -- and, building those, for the states they refer to one level
 * down, and so on for (lc_max - images_level) levels.  That closure is 60 .. 150 of the 1200 .. 2700 luminance states
 * of a 720p / 1080p frame (measured with the oracle), the same values as the full tables hold for them, and the
 * tables of a chroma block were 60 % of a colour frame.
 *
 * F.hits[s] (free once the chroma list is chosen): low half = levels at which the entries of s are needed for the
 * chroma list's sake (static, op_chroma_pool), high half = the same for the block at hand (+ the luminance states
 * of the block's subtree).  Bit k <-> level images_level + k; bit 0 = the level-images_level dots (d5, d4). */
__device__ __forceinline__ int hits_ld(const DevFrame &F, int s) { return __hip_atomic_load(&F.hits[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

/* one step of the closure on half `sft` (0 / 16): what needs level k of s needs level k - 1 of the tree children
 * and edge targets of s */
__device__ void chroma_need_step(const DevFrame &__restrict__ F, Sh &__restrict__ sh, int sft)
{
    const int n = sh.ystates;
    for (int s = threadIdx.x; s < n; s += B) {
        const int m = ((hits_ld(F, s) >> sft) & 0xffff) >> 1;
        if (!m) continue;
        for (int l = 0; l < 2; l++) {
            int d = TREE(F, s, l);
            if (d != RANGE_) __hip_atomic_fetch_or(&F.hits[d], m << sft, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int e = 0; (d = INTO(F, s, l, e)) != NOEDGE; e++)
                __hip_atomic_fetch_or(&F.hits[d], m << sft, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
}

/* end of op_chroma_pool: the part of the closure that is the same for every block (the chroma list) */
__device__ void chroma_need_static(const DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    const int tid = threadIdx.x, n = sh.ystates, NB = F.lc_max - F.images_level;
    __syncthreads();
    for (int s = tid; s < n; s += B) __hip_atomic_store(&F.hits[s], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    for (int i = tid; i < (int) sh.pool.n; i += B)
        __hip_atomic_store(&F.hits[F.pool_states[i]], (1 << (NB + 1)) - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    for (int it = 0; it < NB; it++) chroma_need_step(F, sh, 0);
}

/* per block: + the luminance states of the block's subtree (the co-located states of its ranges), compacted into sh.cl.
 * false: more states than sh.cl holds -- the caller builds the full tables */
__device__ bool chroma_need_block(const DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    const int tid = threadIdx.x, n = sh.ystates, il = F.images_level, NB = F.lc_max - il;
    const int y = sh.st[sh.sp].y_state;
    for (int s = tid; s < n; s += B) {
        const int v = hits_ld(F, s) & 0xffff;
        __hip_atomic_store(&F.hits[s], v | (v << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) sh.cln = 0;
    __syncthreads();
    if (y != RANGE_) {
        /* nodes of the block's subtree, heap order.  The block is of level F.lc_max (op_init_range builds no other)
         * and its ranges go down to the band's running minimum level, which the ratchet keeps at or below lc_max
         * (band_advance); clamped all the same: a negative shift count would be undefined */
        const int dlv = F.lc_max > sh.lc_min ? F.lc_max - sh.lc_min : 0;
        const int nheap = (2 << dlv) - 1;
        for (int h = tid; h < nheap; h += B) {
            const int depth = 31 - __clz(h + 1);
            int node = y;
            for (int b = depth - 1; b >= 0 && node != RANGE_; b--) node = TREE(F, node, ((h + 1) >> b) & 1);
            if (node == RANGE_) continue;
            const int lv = F.lc_max - depth, k = lv > il ? lv - il : 0;
            __hip_atomic_fetch_or(&F.hits[node], 1 << (16 + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        for (int it = 0; it < NB; it++) chroma_need_step(F, sh, 16);
    }
    for (int s = tid; s < n; s += B)
        if ((hits_ld(F, s) >> 16) && F.domain_type[s]) {
            const int i = atomicAdd(&sh.cln, 1);
            if (i < FC_CLMAX) sh.cl[i] = (short) s;
        }
    __syncthreads();
    const int cap = F.chroma_cl_cap > 0 && F.chroma_cl_cap < FC_CLMAX ? F.chroma_cl_cap : FC_CLMAX;
    return sh.cln <= cap;
}

/* op_d5 for the states of sh.cl that need their level-images_level dots: (state, group of eight addresses) items */
__device__ void op_d5_sparse(const DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    const int tid = threadIdx.x, P = F.P, NA = F.NA, ngrp = (NA + 7) / 8;
    float *const D5 = ACT_D5(F, sh);
    for (int it = tid; it < sh.cln * ngrp; it += B) {
        const int s = sh.cl[it / ngrp], a0 = (it % ngrp) * 8;
        if (!((hits_ld(F, s) >> 16) & 1)) continue;
        float v[32];
#pragma unroll
        for (int k = 0; k < 32; k++) v[k] = F.imgT[(size_t) k * P + s];
        for (int a = a0; a < a0 + 8 && a < NA; a++) {
            float ip = 0;
#pragma unroll
            for (int k = 0; k < 32; k++) ip += sh.pixels[a * 32 + k] * v[k];      /* codec/ip.c:268-295, sequential */
            D5[D5_AT(P, NA, a, s)] = ip;
        }
    }
#if FC_VARIANT_BIG
    if (F.gl0 < F.images_level) {
        float *const D4 = ACT_D4(F, sh);
        for (int i = tid; i < sh.cln; i += B) {
            const int s = sh.cl[i];
            if (!((hits_ld(F, s) >> 16) & 1)) continue;
            float v4[16];
#pragma unroll
            for (int k = 0; k < 16; k++) v4[k] = F.imgT4[(size_t) k * P + s];
            for (int a = 0; a < 2 * NA; a++) {
                float ip = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) ip += sh.pixels[a * 16 + k] * v4[k];
                D4[(size_t) a * P + s] = ip;
            }
        }
    }
#endif
}

/* op_ipis for the (state, level) pairs of the closure: per level the items (state, slot); the additions of an entry
 * in the reference's order -- label 0 {tree child, edges}, label 1 {...} onto zero (codec/ip.c:104-146).
 * Slot-major only, sources and results, also where op_ipis_t keeps a state-major copy (FC_IPT): the two never mix
 * inside a block -- a sparse block is built by this function alone, and the only later writer of a block's entries,
 * OP_IPIS_INCR, is not issued in a chroma band (`!sh.band', fc_serial.inc). */
__device__ void op_ipis_sparse(const DevFrame &__restrict__ F, Sh &__restrict__ sh, int level)
{
    const int tid = threadIdx.x, il = F.images_level, P = F.P;
    float *const ipis = ACT_IPIS(F, sh);
    const float *const d5 = ACT_D5(F, sh);
    for (int lv = il + 1; lv <= level; lv++) {
        const int delta = level - lv, cnt = 1 << delta, slot0 = cnt - 1, k = lv - il;
        const bool first = lv == il + 1;
        for (int it = tid; it < sh.cln * cnt; it += B) {
            const int s = sh.cl[it >> delta], j = it & (cnt - 1);
            if (!((hits_ld(F, s) >> (16 + k)) & 1)) continue;
            float acc = 0;
            for (int l = 0; l < 2; l++) {
                int d = TREE(F, s, l);
                /* the entry of state d one level down: sub-block 2 j + l of the level below */
#if FC_D5T
#define SRC(d) (first ? d5[D5_AT(P, F.NA, j * 2 + l, (d))] : ipis[(size_t) ((slot0 * 2 + 1) + j * 2 + l) * P + (d)])
#else
#define SRC(d) (first ? d5[(size_t) (j * 2 + l) * P + (d)] : ipis[(size_t) ((slot0 * 2 + 1) + j * 2 + l) * P + (d)])
#endif
                if (d != RANGE_) acc += SRC(d);
                for (int e = 0; (d = INTO(F, s, l, e)) != NOEDGE; e++) acc += WEIGHT(F, s, l, e) * SRC(d);
#undef SRC
            }
            ipis[(size_t) (slot0 + j) * P + s] = acc;
        }
        __syncthreads();
    }
}
#endif

/* codec/subdivide.c:504-541,612-644 */
/* from: the entries of the states below it are in the tables already (FC_SPEC: a table worker has
 * computed them ahead of the chain); otherwise 0 */
__device__ __noinline__ void op_init_range(DevFrame &__restrict__ F, Sh &__restrict__ sh, int x0, int y0, int from)
{
    const int tid = threadIdx.x;
    const int level = F.lc_max, npx = 1 << level;
    const int16_t *plane = F.pix16 + (size_t) sh.band * F.plane;
#if FC_VARIANT_BIG
    if (F.frame_type && sh.band) plane = F.pix_chroma + (size_t) (sh.band - 1) * F.plane;
#endif
    {   /* all pixel loads of the lane in flight: unconditional loads at clamped coordinates,
         * the outside of the image is zeroed afterwards (codec/subdivide.c:504-541) */
        constexpr int NIT = FC_PIXELS / B;
        GLOBAL_AS const int16_t *const gplane = uniform_ptr(plane);      /* a plane is < 2^31 pixels */
        const int width = F.width, height = F.height;
        int raw[NIT];
        bool inside[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = tid + it * B;
            unsigned xo = 0, yo = 0;
#pragma unroll
            for (int b = 0; b < 13; b++) {
                yo |= ((i >> (2 * b)) & 1u) << b;         /* even bits: rows (mask 0x555555)   */
                xo |= ((i >> (2 * b + 1)) & 1u) << b;     /* odd bits: columns (mask 0xaaaaaa) */
            }
            const int x = x0 + (int) xo, y = y0 + (int) yo;
            inside[it] = i < npx && y < height && x < width;
            const int xc = x < width ? x : width - 1, yc = y < height ? y : height - 1;
            raw[it] = ldg(gplane, (unsigned) (yc * width + xc));
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = tid + it * B;
            if (i < npx) sh.pixels[i] = inside[it] ? (float) (raw[it] / 16) : 0.0f;
        }
    }
    __syncthreads();
#if !FC_SPEC
    /* chroma bands: entries for the states somebody reads only (chroma_need_block) */
    const bool sparse = sh.band && !F.bx && F.chroma_sparse && chroma_need_block(F, sh);
#else
    const bool sparse = false;
#endif
#if FC_VARIANT_BIG
    /* the helpers start on the block while this workgroup sums the norms (LDS only) */
    const int coopD = sparse ? 0 : coop_publish(F, sh, level, from);
#endif
    /* squared norms of every sub-block, sequential as codec/approx.c:388-389 */
    for (int slot = tid; slot < F.NS; slot += B) {
        int depth = 31 - __clz(slot + 1);
        int lv = level - depth, size = 1 << lv;
        int adr = slot + 1 - (1 << depth);
        float nrm = 0;
        const float *px = sh.pixels + adr * size;
        for (int k = 0; k < size; k += 8) {        /* size >= 64: 8 LDS reads in flight, */
            float p0 = px[k], p1 = px[k + 1], p2 = px[k + 2], p3 = px[k + 3];   /* adds stay */
            float p4 = px[k + 4], p5 = px[k + 5], p6 = px[k + 6], p7 = px[k + 7]; /* sequential */
            nrm += p0 * p0; nrm += p1 * p1; nrm += p2 * p2; nrm += p3 * p3;
            nrm += p4 * p4; nrm += p5 * p5; nrm += p6 * p6; nrm += p7 * p7;
        }
        sh.norms[slot] = nrm;              /* LDS: read by lane 0 at the start of every search */
    }
#ifdef FC_SERIAL_PROFILE
    unsigned long long tp0 = wall_clock64();
#endif
#if !FC_SPEC
    if (sparse) {
        op_d5_sparse(F, sh);
        __syncthreads();
        op_ipis_sparse(F, sh, level);
        if (tid == 0) {          /* what was built, not what the reference builds: cln states */
            sh.cnt.bytes_img += (unsigned long long) sh.cln * (4ull * 32 + 4ull * F.NS) + 4ull * npx;
            sh.cnt.n_blocks++;
        }
        return;
    }
#endif
#if FC_VARIANT_BIG
    if (coopD) {
        coop_finish(F, sh, level, from, coopD);
        op_ipis(F, sh, 0, 0, level, from, level - coopD + 1);
    } else {
#endif
    op_d5(F, sh, from, table_states(sh), F.NA, 2 * F.NA);
    __syncthreads();
#ifdef FC_SERIAL_PROFILE
    if (tid == 0) { unsigned long long t = wall_clock64(); sh.tk_init[0] += t - tp0; tp0 = t; }
#endif
    op_ipis(F, sh, 0, 0, level, from);
#if FC_VARIANT_BIG
    }
#endif
#ifdef FC_SERIAL_PROFILE
    if (tid == 0) sh.tk_init[1] += wall_clock64() - tp0;
#endif
    if (tid == 0) {
        sh.cnt.bytes_img += (unsigned long long) table_states(sh) * (4ull * 32 + 4ull * F.NS) + 4ull * npx;
        sh.cnt.n_blocks++;
    }
}
