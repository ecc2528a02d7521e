/*
 *  fc_access.inc -- small helpers (rtob_dev, bits_bin_code, qac_shift, ldg, stg); the hand-offs
 *  between workgroups (publish_release, take_acquire); access to the Gram and image tables
 *  (gram_*, image_elem, BxView).
 *
 *  Reference: rate models lib/rpf.c:59-169, lib/misc.c:223-244; inner-product tables
 *  codec/ip.c:46-323.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

/* ------------------------------------------------------------------ small helpers */

__device__ __forceinline__ unsigned width_of_level(int l)  { return 1u << (l >> 1); }
__device__ __forceinline__ unsigned height_of_level(int l) { return 1u << ((l + 1) >> 1); }

/* lib/rpf.c:59-112 (x86 masks variable shift counts to 5 bits; so does this) */
__device__ int rtob_dev(float f, int mant, float range)
{
    f /= range;
    unsigned bits = __float_as_uint(f);
    unsigned m = bits & 0x7fffffu;
    int e = (int) ((bits >> 23) & 0xffu) - 126;
    int sign = (int) (bits >> 31);
    m = (m >> 1) | (1u << 22);
    if (e > 0) m <<= ((unsigned) e & 31u);
    else       m >>= ((unsigned) (-e) & 31u);
    m >>= (23 - mant - 1);
    m += 1;
    m >>= 1;
    if (m == 0) return -1;
    if (m >= (1u << mant)) return sign;
    return (int) (((m & ((1u << mant) - 1)) << 1) | (unsigned) sign);
}

/* lib/misc.c:223-244 */
__device__ __forceinline__ unsigned bits_bin_code(unsigned value, unsigned maxval)
{
    unsigned k = 31u - (unsigned) __clz((int) (maxval + 1));
    unsigned r = (maxval + 1) - (1u << k);
    return value < maxval + 1 - 2 * r ? k : k + 1;
}

/* probability index -> shift n of the quasi-arithmetic model (domain-pool.c:970-999) */
__device__ __forceinline__ int qac_shift(int index)
{
    int n = 1, start = 0;
    while (index >= start + (1 << n)) { start += 1 << n; n++; }
    return n;
}

/* Out-of-line functions get the frame descriptor through a generic reference, so every table
 * pointer they read is per-lane data to the compiler (64-bit address arithmetic in VGPRs for
 * each access).  The pointers ARE uniform: moving them to scalar registers leaves one 32-bit
 * lane offset per access. */
#define GLOBAL_AS __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ GLOBAL_AS T *uniform_ptr(T *p)
{
    unsigned long long v = (unsigned long long) p;
    unsigned lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) v);
    unsigned hi = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) (v >> 32));
    /* known to be HBM (never LDS/scratch): global_load with a scalar base, not flat_load */
    return (GLOBAL_AS T *) (((unsigned long long) hi << 32) | lo);
}

/* element i of a table behind a scalar base: the byte offset is formed in 32 bits so that
 * the access is `global_load v, v_off, s[base:base+1]` (tables are < 4 GB apart from gram,
 * which is not accessed this way) */
template <typename T>
__device__ __forceinline__ T ldg(GLOBAL_AS const T *base, unsigned i)
{
    return *(GLOBAL_AS const T *) ((GLOBAL_AS const char *) base + i * (unsigned) sizeof(T));
}
template <typename T>
__device__ __forceinline__ void stg(GLOBAL_AS T *base, unsigned i, T v)
{
    *(GLOBAL_AS T *) ((GLOBAL_AS char *) base + i * (unsigned) sizeof(T)) = v;
}

/* ------------------------------------------------------------------ hand-offs between workgroups
 *
 * Per-XCD L2s are not coherent with each other and a CU's vector L1 is never refreshed by another CU's stores
 * (MI355X_MICROARCH.md, "inter-workgroup visibility"): data for another workgroup is PUBLISHED -- every wave drains its
 * stores, the workgroup meets, ONE lane writes the XCD L2's dirty lines back (agent-scope release) and only then stores
 * the flag -- and TAKEN by polling the flag relaxed, ONE agent-scope acquire (drops this CU's L1) and a barrier before
 * the plain loads.  The explicit waits are not decoration: ROCm 7.2 drops the `s_waitcnt vmcnt(0)' behind `buffer_wbl2'
 * whenever its scoreboard says the publishing wave has nothing outstanding, and the flag then overtakes the write-back
 * (round 6: the append helpers read the PREVIOUS row's descriptor until the wait was written out). */
#define WAVE_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
/* lane 0 of a workgroup whose waves have all drained and met (WAVE_DRAIN(); __syncthreads();): after this a relaxed
 * agent-scope store / fetch_add of the flag publishes everything the workgroup has written */
__device__ __forceinline__ void publish_release(void)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
/* the taker's side, one lane, after it has seen the flag (relaxed): nothing stale of the publisher's data in this CU's L1 */
__device__ __forceinline__ void take_acquire(void)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

/* ------------------------------------------------------------------ table access */

/* Gram tables, two layouts (frame_coder.h): full symmetric P x P per level, or -- FC_GRAM_TRI,
 * the build for frames whose full tables HBM cannot hold for every CU (4K) -- the lower triangle
 * with packed rows, <a, b> with a >= b at TRI(a) + b.  The levels are gram_ls floats apart. */
#ifndef FC_GRAM_TRI
#define FC_GRAM_TRI 0
#endif
#define TRI(a)       ((unsigned) (a) * ((unsigned) (a) + 1u) / 2u)
#define GROW(a, P)   (FC_GRAM_TRI ? TRI(a) : (unsigned) (a) * (unsigned) (P))     /* start of row a in a level */
#define GRAM(F, q)   ((F).gram + (size_t) (q) * (F).gram_ls)
/* the same through the LDS copy of the table base (no descriptor read on the hot path) */
#define PGRAM(sh, q)  ((sh).par.gram + (size_t) (q) * (sh).par.gram_ls)
#define TREE(F, s, l)        ((F).tree[(l) * (F).PA + (s)])
#define INTO(F, s, l, e)     ((F).into[((l) * 6 + (e)) * (F).PA + (s)])
#define WEIGHT(F, s, l, e)   ((F).weight[((l) * 6 + (e)) * (F).PA + (s)])

__device__ __forceinline__ float gram_load(const float *G, int P, int a, int b, int flim);
#define NOFLIM 0x7fffffff        /* every entry is stored both ways (the basis states) */

/* one Gram entry at table level q >= 1 from level q-1 (codec/ip.c:213-257) */
__device__ float gram_entry(const DevFrame &F, int q, int s1, int s2)
{
    const float *G = GRAM(F, q - 1);
    const int P = F.P;
    float ip = 0;
    for (int label = 0; label < 2; label++) {
        int d1, d2;
        float sum;
        int t2 = TREE(F, s2, label);
        if ((d1 = TREE(F, s1, label)) != RANGE_) {
            sum = 0;
            if (t2 != RANGE_) sum = gram_load(G, P, d1, t2, NOFLIM);
            for (int e2 = 0; (d2 = INTO(F, s2, label, e2)) != NOEDGE; e2++)
                sum += WEIGHT(F, s2, label, e2) * gram_load(G, P, d1, d2, NOFLIM);
            ip += sum;
        }
        for (int e1 = 0; (d1 = INTO(F, s1, label, e1)) != NOEDGE; e1++) {
            float w1 = WEIGHT(F, s1, label, e1);
            sum = 0;
            if (t2 != RANGE_) sum = gram_load(G, P, d1, t2, NOFLIM);
            for (int e2 = 0; (d2 = INTO(F, s2, label, e2)) != NOEDGE; e2++)
                sum += WEIGHT(F, s2, label, e2) * gram_load(G, P, d1, d2, NOFLIM);
            ip += w1 * sum;
        }
    }
    return ip;
}

/* level-images_level Gram entry: plain sequential dot (codec/ip.c:297-323) */
__device__ float gram_dot(const DevFrame &F, int s1, int s2)
{
    const int n = 1 << F.images_level;
    float ip = 0;
    for (int k = 0; k < n; k++)
        ip += F.imgT[(size_t) k * F.P + s1] * F.imgT[(size_t) k * F.P + s2];
    return ip;
}

#if FC_VARIANT_BIG
/* the same one level lower (block levels down to 4) */
__device__ float gram_dot4(const DevFrame &F, int s1, int s2)
{
    const int n = 1 << (F.images_level - 1);
    float ip = 0;
    for (int k = 0; k < n; k++)
        ip += F.imgT4[(size_t) k * F.P + s1] * F.imgT4[(size_t) k * F.P + s2];
    return ip;
}
#endif

/* s >= t */
__device__ void gram_store(const DevFrame &F, int q, int s, int t, float v)
{
    float *G = GRAM(F, q);
    G[GROW(s, F.P) + (unsigned) t] = v;
#if !FC_GRAM_TRI
    G[(size_t) t * F.P + s] = v;
#else
    if (t < FC_TRI_HOT && t < s) F.gcol[((size_t) q * FC_TRI_HOT + t) * F.P + s] = v;
#endif
    if (s == t) F.diag[(size_t) q * F.P + s] = v;
}

/*
 *  Symmetric Gram tables without scattered writes.  A new state s writes only its ROW
 *  (entries t <= s, contiguous).  The mirrored entries G[t][s] -- one 4-byte store per
 *  128-byte line when written directly, i.e. 32x write amplification in HBM -- are produced
 *  later in blocks of GRAM_FB states by gram_flush(): 128-byte segments, full lines.
 *  Invariant: with flim = sh.flim, G[a][b] is stored if b <= a or max(a, b) < flim; an entry
 *  outside that set is read through its mirror image.
 */
#define GRAM_FB 32

/* position of <a, b> in a level.  Triangle: whichever of the two is larger names the row. */
__device__ __forceinline__ unsigned gram_idx(int P, int a, int b, int flim)
{
#if FC_GRAM_TRI
    return a >= b ? TRI(a) + (unsigned) b : TRI(b) + (unsigned) a;
#else
    const bool mirror = b > a && b >= flim;
    return mirror ? (unsigned) b * (unsigned) P + (unsigned) a : (unsigned) a * (unsigned) P + (unsigned) b;
#endif
}
__device__ __forceinline__ float gram_load(const float *G, int P, int a, int b, int flim)
{
    return G[gram_idx(P, a, b, flim)];
}

#if FC_GRAM_TRI
/*
 *  The triangle.  A new state writes its row (entries t <= s, contiguous) and nothing else; the
 *  sweep of a matching-pursuit step reads the chosen state's row up to the diagonal and, for the
 *  candidates behind it, the chosen state's COLUMN -- one 4-byte gather per candidate, a whole
 *  line of HBM traffic each.  Half the memory per frame: at 4K, where the full tables allow slabs
 *  for only half the CUs, that doubles the frames in flight (16.2 -> 24.6 frames/s); at 1080p,
 *  where every CU has its four frames anyway, the gathers cost 28 % (547 -> 392 frames/s) --
 *  which is why the layout is a property of the kernel build and the launcher picks by memory.
 */
__device__ __forceinline__ void gram_flush(const DevFrame &, Sh &, int) { }
#else

__device__ void gram_flush(const DevFrame &__restrict__ F, Sh &__restrict__ sh, int upto)
{
    const int tid = threadIdx.x, P = __builtin_amdgcn_readfirstlane(F.P);
    int flim = sh.flim;
#if FC_SPEC
    if (sh.sl.role > 0) return;      /* a verifier reads what its own states have in their own rows */
#endif
    if (upto - flim < GRAM_FB) return;                      /* uniform */
    __syncthreads();                                        /* the rows are complete */
    while (upto - flim >= GRAM_FB) {
        for (int q = 0; q < F.NL; q++) {
            /* (a level is P x P floats, < 4 GB: 32-bit element offsets behind a scalar base) */
            GLOBAL_AS float *G = uniform_ptr(GRAM(F, q));
            for (int t = tid; t < flim + GRAM_FB; t += B) {
                if (t < flim) {
                    float v[GRAM_FB];
#pragma unroll
                    for (int j = 0; j < GRAM_FB; j++) v[j] = ldg((GLOBAL_AS const float *) G, (unsigned) ((flim + j) * P + t));
                    typedef float f4 __attribute__((ext_vector_type(4)));
                    GLOBAL_AS f4 *dst = (GLOBAL_AS f4 *) ((GLOBAL_AS char *) G + (unsigned) (t * P + flim) * 4u);
#pragma unroll
                    for (int j = 0; j < GRAM_FB / 4; j++) {
                        const f4 w = { v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3] };
                        dst[j] = w;
                    }
                } else {
                    for (int j = t - flim + 1; j < GRAM_FB; j++)
                        stg(G, (unsigned) (t * P + flim + j), ldg((GLOBAL_AS const float *) G, (unsigned) ((flim + j) * P + t)));
                }
            }
        }
        flim += GRAM_FB;
    }
    __syncthreads();
    if (tid == 0) sh.flim = flim;
}
#endif

/* state image element (codec/control.c:205-258): level l >= 1, position i */
__device__ float image_elem(const DevFrame &F, int s, int l, int i)
{
    int half = 1 << (l - 1);
    int label = i >= half;
    int pos = i - label * half;
    int base = half - 1;                 /* address_of_level(l-1) */
    float v = 0;
    int dom;
    if ((dom = TREE(F, s, label)) != RANGE_) v = F.img[(size_t) dom * F.NI + base + pos];
    for (int e = 0; (dom = INTO(F, s, label, e)) != NOEDGE; e++)
        v += F.img[(size_t) dom * F.NI + base + pos] * WEIGHT(F, s, label, e);
    return v;
}

#if FC_VARIANT_BIG
/* ---- a basis that travels as the memory image of its rows (DevFrame.bx; data/medium.fco, large.fco) ----
 * The edge list of (state, label) starts at entry (2 state + label) * 6 and ends at the first NO_EDGE -- beyond
 * the row's own six entries where the reference's append_edge ran on into the next row (codec/wfalib.c:253-273).
 * Basis states have no tree children.  Their rows in the automaton arrays of the slab stay empty: the table
 * passes below take the basis states' terms from here, in the reference's order of additions. */
struct BxView { int nb; const float *final_d; const int *dtype; const float *w; const int16_t *into; };
__device__ __forceinline__ BxView bx_view(const DevFrame &F)
{
    BxView v;
    const int *b = F.bx;
    v.nb = b[0];
    v.final_d = (const float *) (b + 4); v.dtype = b + 4 + v.nb; v.w = (const float *) (b + 4 + 2 * v.nb);
    v.into = (const int16_t *) (b + 4 + 2 * v.nb + b[1]);
    return v;
}

/* image_elem() of a basis state */
__device__ float image_elem_bx(const DevFrame &F, const BxView &V, int s, int l, int i)
{
    const int half = 1 << (l - 1), label = i >= half, pos = i - label * half, base = half - 1;
    float v = 0;
    int dom;
    for (int e = (s * 2 + label) * 6; (dom = V.into[e]) != NOEDGE; e++)
        v += F.img[(size_t) dom * F.NI + base + pos] * V.w[e];
    return v;
}

/* gram_entry() of two basis states */
__device__ float gram_entry_bx(const DevFrame &F, const BxView &V, int q, int s1, int s2)
{
    const float *G = GRAM(F, q - 1);
    const int P = F.P;
    float ip = 0;
    for (int label = 0; label < 2; label++) {
        int d1, d2;
        for (int e1 = (s1 * 2 + label) * 6; (d1 = V.into[e1]) != NOEDGE; e1++) {
            float sum = 0;
            for (int e2 = (s2 * 2 + label) * 6; (d2 = V.into[e2]) != NOEDGE; e2++)
                sum += V.w[e2] * gram_load(G, P, d1, d2, NOFLIM);
            ip += V.w[e1] * sum;
        }
    }
    return ip;
}
#endif
