/*
 *  rccl_gather.inc -- the finished streams of all ranks onto one rank (included by core_hip.cpp): one process per
 *  GPU, RCCL taken from the process at run time.
 */

/* ------------------------------------------------------------------ gather of the streams over RCCL
 *
 * One process per GPU (SURVEY.md 8e, BASELINE config 4): every rank encodes its share of the frames -- frame i of the
 * job on rank i mod W -- and the finished byte strings (kilobytes per frame) meet on one rank: two small all-gathers for
 * the counts and lengths, one padded all-gather for the payloads, over xGMI.  No data-path collective exists; this is
 * the only communication of the job.  RCCL is NOT a link-time dependency of the library: the entry points are taken
 * from the copy the process already has (the one that made the caller's communicator), else from librccl.so. */
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, void *);
typedef const char *(*nccl_errstr_fn)(int);
enum { FA_NCCL_UINT8 = 1, FA_NCCL_UINT64 = 5 };          /* ncclDataType_t, rccl.h */

extern "C" int fiasco_amd_rccl_gather(void *comm, void *stream_, int rank, int world, int root,
                                      unsigned n_local, const unsigned char *const *data, const size_t *len,
                                      unsigned char ***all, size_t **all_len, unsigned *n_all)
{
    hipStream_t stream = (hipStream_t) stream_;
    if (all) *all = nullptr;
    if (all_len) *all_len = nullptr;
    if (n_all) *n_all = 0;
    if (!comm || world < 1 || rank < 0 || rank >= world || root < 0 || root >= world || (n_local && (!data || !len))) {
        fa_set_error("fiasco_amd_rccl_gather: bad arguments");
        return 0;
    }
    static nccl_allgather_fn allgather = nullptr;
    static nccl_errstr_fn errstr = nullptr;
    if (!allgather) {
        allgather = (nccl_allgather_fn) dlsym(RTLD_DEFAULT, "ncclAllGather");
        errstr = (nccl_errstr_fn) dlsym(RTLD_DEFAULT, "ncclGetErrorString");
        if (!allgather) {
            void *h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (h) { allgather = (nccl_allgather_fn) dlsym(h, "ncclAllGather"); errstr = (nccl_errstr_fn) dlsym(h, "ncclGetErrorString"); }
        }
        if (!allgather) { fa_set_error("fiasco_amd_rccl_gather: no RCCL in this process (librccl.so)"); return 0; }
    }
    /* Failure discipline: a collective that one rank skips hangs every other rank.  So every rank takes part in
     * every collective the OTHERS will enter: a rank-local failure travels as a flag in the next message -- word 2 of
     * the counts, then a status round after the payload buffers have been allocated (whose size no rank knows before
     * the counts are in) -- and all ranks, looking at the same gathered words, fail TOGETHER before the all-gather of
     * the streams.  The one exception is the first allocation (24 (W + 1) bytes): a rank that cannot get that cannot
     * signal anything.  The root's return value is the job's; a rank that is not the root returns 1 once its part is
     * delivered. */
    unsigned long long *d_u64 = nullptr;
    unsigned char *d_pay = nullptr;
    int ok = 1, rc = 0;
    const size_t W = (size_t) world;
    std::vector<unsigned long long> h_cnt(W * 3), h_st(W * 3);
#define GCHECK(call, what) do { if ((call) != hipSuccess) { if (ok) fa_set_error("fiasco_amd_rccl_gather: %s: %s", what, hipGetErrorString(hipGetLastError())); ok = 0; } } while (0)
#define NCHECK(call, what) do { if ((rc = (call)) != 0) { if (ok) fa_set_error("fiasco_amd_rccl_gather: %s: %s", what, errstr ? errstr(rc) : "RCCL error"); ok = 0; } } while (0)
    /* 1. counts, total bytes and failure flag of every rank */
    unsigned long long mine[3] = { n_local, 0, 0 };
    for (unsigned i = 0; i < n_local; i++) mine[1] += len[i];
    if (hipMalloc((void **) &d_u64, sizeof(unsigned long long) * 3 * (W + 1)) != hipSuccess) {
        fa_set_error("fiasco_amd_rccl_gather: hipMalloc: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }
    GCHECK(hipMemcpyAsync(d_u64 + 3 * W, mine, sizeof mine, hipMemcpyHostToDevice, stream), "upload");
    NCHECK(allgather(d_u64 + 3 * W, d_u64, 3, FA_NCCL_UINT64, comm, stream), "all-gather of the counts");
    GCHECK(hipMemcpyAsync(h_cnt.data(), d_u64, sizeof(unsigned long long) * 3 * W, hipMemcpyDeviceToHost, stream), "download");
    GCHECK(hipStreamSynchronize(stream), "synchronize");
    size_t maxn = 0, maxb = 0, total = 0;
    if (ok) {
        for (size_t r = 0; r < W; r++) {
            if (h_cnt[3 * r] > maxn) maxn = (size_t) h_cnt[3 * r];
            if (h_cnt[3 * r + 1] > maxb) maxb = (size_t) h_cnt[3 * r + 1];
            total += (size_t) h_cnt[3 * r];
        }
        /* the deal must be round robin (item i on rank i mod W): rank r holds ceil((total - r) / W) streams -- anything
         * else (or garbage from a rank whose upload failed) would be put in the wrong places below; every rank sees the
         * same words and fails alike */
        for (size_t r = 0; r < W; r++) {
            const size_t want = total > r ? (total - r + W - 1) / W : 0;
            if ((size_t) h_cnt[3 * r] != want || h_cnt[3 * r + 2] != 0) {
                fa_set_error(h_cnt[3 * r + 2] ? "fiasco_amd_rccl_gather: rank %d reported a failure"
                                              : "fiasco_amd_rccl_gather: rank %d holds %llu of %llu streams: the frames were not dealt round robin",
                             (int) r, (unsigned long long) h_cnt[3 * r], (unsigned long long) total);
                ok = 0;
                break;
            }
        }
    }
    /* 2. per rank: maxn lengths + maxb payload bytes (padded).  Buffers first, then a status round: nobody enters the
     * big all-gather unless everybody can (a rank whose step 1 failed locally reports that here too) */
    const size_t slot = ok ? align_up(maxn * 8 + maxb, 16) : 0;
    std::vector<unsigned char> h_send, h_recv;
    unsigned long long st[3] = { ok ? 0ull : 1ull, 0, 0 };
    if (ok && slot) {
        try { h_send.assign(slot, 0); if (rank == root) h_recv.resize(slot * W); } catch (...) { st[0] = 1; }
        if (!st[0] && hipMalloc((void **) &d_pay, slot * (W + 1)) != hipSuccess) { (void) hipGetLastError(); d_pay = nullptr; st[0] = 1; }
        if (st[0]) { fa_set_error("fiasco_amd_rccl_gather: out of memory for %zu bytes per rank", slot); ok = 0; }
    }
    {
        int ok2 = 1;                                   /* the status round itself; `ok' keeps the first message */
        if (hipMemcpyAsync(d_u64 + 3 * W, st, sizeof st, hipMemcpyHostToDevice, stream) != hipSuccess) ok2 = 0;
        if (allgather(d_u64 + 3 * W, d_u64, 3, FA_NCCL_UINT64, comm, stream) != 0) ok2 = 0;
        if (hipMemcpyAsync(h_st.data(), d_u64, sizeof(unsigned long long) * 3 * W, hipMemcpyDeviceToHost, stream) != hipSuccess) ok2 = 0;
        if (hipStreamSynchronize(stream) != hipSuccess) ok2 = 0;
        if (!ok2) { (void) hipGetLastError(); if (ok) fa_set_error("fiasco_amd_rccl_gather: the status round failed"); ok = 0; }
        for (size_t r = 0; ok2 && r < W; r++)
            if (h_st[3 * r]) { if (ok) fa_set_error("fiasco_amd_rccl_gather: rank %d cannot take part (see its message)", (int) r); ok = 0; break; }
    }
    if (ok && slot) {
        size_t o = maxn * 8;
        for (unsigned i = 0; i < n_local; i++) {
            const unsigned long long l = len[i];
            memcpy(h_send.data() + (size_t) i * 8, &l, 8);
            memcpy(h_send.data() + o, data[i], len[i]);
            o += len[i];
        }
        GCHECK(hipMemcpyAsync(d_pay + slot * W, h_send.data(), slot, hipMemcpyHostToDevice, stream), "upload");
        NCHECK(allgather(d_pay + slot * W, d_pay, slot, FA_NCCL_UINT8, comm, stream), "all-gather of the streams");
        if (rank == root) GCHECK(hipMemcpyAsync(h_recv.data(), d_pay, slot * W, hipMemcpyDeviceToHost, stream), "download");
        GCHECK(hipStreamSynchronize(stream), "synchronize");
    }
    if (d_pay) (void) hipFree(d_pay);
    if (d_u64) (void) hipFree(d_u64);
#undef GCHECK
#undef NCHECK
    if (!ok) return 0;
    if (rank != root || !all || !all_len || !n_all) return 1;
    /* 3. the root: stream k of rank r is item r + k * world of the job (the round-robin deal, checked above) */
    unsigned char **out = (unsigned char **) calloc(total ? total : 1, sizeof *out);
    size_t *olen = (size_t *) calloc(total ? total : 1, sizeof *olen);
    int oom = !out || !olen;
    for (size_t r = 0; !oom && r < W; r++) {
        const unsigned char *base = h_recv.data() + slot * r;
        size_t o = maxn * 8;
        for (size_t k = 0; !oom && k < (size_t) h_cnt[3 * r]; k++) {
            unsigned long long l;
            memcpy(&l, base + k * 8, 8);
            const size_t item = r + k * W;               /* < total: the deal was checked */
            out[item] = (unsigned char *) malloc(l ? (size_t) l : 1);
            if (!out[item]) { oom = 1; break; }
            memcpy(out[item], base + o, (size_t) l);
            olen[item] = (size_t) l;
            o += (size_t) l;
        }
    }
    if (oom) {
        if (out) for (size_t i = 0; i < total; i++) free(out[i]);
        free(out); free(olen);
        fa_set_error("fiasco_amd_rccl_gather: out of memory");
        return 0;
    }
    *all = out; *all_len = olen; *n_all = (unsigned) total;
    return 1;
}
