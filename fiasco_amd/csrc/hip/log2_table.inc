/*
 *  log2_table.inc -- log2 of a probability on the device against the host's (included by core_hip.cpp): the self
 *  test kernel and its comparison on the host, the table of corrections the frame kernel looks up (Log2Patch of the
 *  share's DevState, DevFrame.l2_*), how it is built and kept in a cache file.
 */

/* ------------------------------------------------------------------ log2 self test
 *
 * The rate models price symbols with double log2 of a float probability p = count / (float)
 * total (codec/coeff.c:232-237, codec/domain-pool.c:772, codec/bintree.c:67).  The host side
 * of the reference evaluates it with glibc, the device with ROCm's ocml; bit parity of the
 * streams needs both to return the same DOUBLE for every argument that can occur.  Every such
 * argument is a float in (0, 1] (and 1 - p is one in [0, 1)), so the claim can be checked
 * exhaustively: this entry evaluates log2((double) p) on the device for all floats of an
 * exponent range and compares the doubles bit for bit with glibc's on the host. */

__global__ void selftest_log2_kernel(unsigned first_bits, unsigned n, double *out, const unsigned *keys,
                                     const double *vals, unsigned mask)
{
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned k = first_bits + i;
    double v = log2((double) __uint_as_float(k));
    if (keys)                                   /* the frame kernel's log2_host(), mp_device.inc */
        for (unsigned h = (k * 2654435761u) & mask, kk; (kk = keys[h]) != 0; h = (h + 1) & mask)
            if (kk == k) { v = vals[h]; break; }
    out[i] = v;
}

/* share t of the comparison on the host (fa_fan_out): what it found */
struct L2Task { const double *dev; unsigned first_bits, n; unsigned long long dd, df; unsigned bad;
                unsigned long long max_ulp;
                std::vector<std::pair<unsigned, double>> *collect; };

static void l2_share(void *ctx, unsigned t, unsigned nt)
{
    L2Task *k = (L2Task *) ctx + t;
    for (unsigned i = t; i < k->n; i += nt) {
        unsigned bits = k->first_bits + i;
        float p; memcpy(&p, &bits, 4);
        double h = log2((double) p), d = k->dev[i];
        if (memcmp(&h, &d, 8) != 0) {
            long long hb, db;
            memcpy(&hb, &h, 8); memcpy(&db, &d, 8);
            unsigned long long dist = (unsigned long long) (hb > db ? hb - db : db - hb);
            if (dist > k->max_ulp) k->max_ulp = dist;
            k->dd++;
            if (k->collect) k->collect->push_back(std::make_pair(bits, h));
            if ((float) -h != (float) -d) { if (!k->df) k->bad = bits; k->df++; }
        }
    }
}

/* the table of host log2 values the kernels use (DevFrame.l2_*), per process */
static std::atomic<unsigned long long> g_l2_max_ulp(0);      /* largest distance seen by the comparisons of the process, in ulps */
extern "C" unsigned long long fiasco_amd_selftest_log2_max_ulp(void) { return g_l2_max_ulp.load(); }

/* compare over the floats with biased exponent in [exp_lo, exp_hi]; with `use_table` the device
 * side goes through the patch table like the frame kernel does; `collect` gathers the
 * arguments that differ together with the host's value */
static int log2_compare(unsigned exp_lo, unsigned exp_hi, bool use_table, unsigned long long *n_checked,
                        unsigned long long *n_double, unsigned long long *n_float, float *first_bad,
                        std::vector<std::pair<unsigned, double>> *collect)
{
    const unsigned CH = 1u << 23;                  /* one binade per launch */
    double *d_out = nullptr, *h_out = nullptr;
    unsigned long long checked = 0, dd = 0, df = 0;
    unsigned bad = 0;
    if (exp_lo < 1) exp_lo = 1;
    if (exp_hi > 127) exp_hi = 127;
    if (hipMalloc((void **) &d_out, (size_t) CH * 8) != hipSuccess
        || hipHostMalloc((void **) &h_out, (size_t) CH * 8, hipHostMallocDefault) != hipSuccess) {
        fa_set_error("selftest: HIP error: %s", hipGetErrorString(hipGetLastError()));
        if (d_out) (void) hipFree(d_out);
        return 0;
    }
    for (unsigned e = exp_lo; e <= exp_hi; e++) {
        const unsigned first = e << 23;
        const unsigned n = e == 127 ? 1u : CH;     /* 1.0 is the largest probability */
        hipLaunchKernelGGL(selftest_log2_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, first, n, d_out,
                           use_table ? g_l2.d_keys : nullptr, use_table ? g_l2.d_vals : nullptr, g_l2.mask);
        if (hipMemcpy(h_out, d_out, (size_t) n * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            fa_set_error("selftest: HIP error: %s", hipGetErrorString(hipGetLastError()));
            (void) hipFree(d_out); (void) hipHostFree(h_out);
            return 0;
        }
        enum { NT = 16 };
        L2Task task[NT];
        std::vector<std::pair<unsigned, double>> part[NT];
        for (unsigned t = 0; t < NT; t++) task[t] = L2Task{ h_out, first, n, 0, 0, 0, 0, collect ? &part[t] : nullptr };
        fa_fan_out(NT, l2_share, task);
        for (unsigned t = 0; t < NT; t++) {
            dd += task[t].dd;
            for (unsigned long long seen = g_l2_max_ulp.load(); task[t].max_ulp > seen; )       /* table builds of two shares may meet here */
                if (g_l2_max_ulp.compare_exchange_weak(seen, task[t].max_ulp)) break;
            if (task[t].df && !df) bad = task[t].bad;
            df += task[t].df;
            if (collect) collect->insert(collect->end(), part[t].begin(), part[t].end());
        }
        checked += n;
    }
    (void) hipFree(d_out); (void) hipHostFree(h_out);
    if (n_checked) *n_checked = checked;
    if (n_double) *n_double = dd;
    if (n_float) *n_float = df;
    if (first_bad) memcpy(first_bad, &bad, 4);
    return 1;
}

/* floats with biased exponent in [exp_lo, exp_hi] (126 = [0.5, 1)); returns 1 when the run
 * completed.  n_double / n_float: arguments whose double result / whose (float) -log2 differ. */
extern "C" int fiasco_amd_selftest_log2(unsigned exp_lo, unsigned exp_hi, unsigned long long *n_checked,
                                        unsigned long long *n_double, unsigned long long *n_float,
                                        float *first_bad)
{
    return log2_compare(exp_lo, exp_hi, false, n_checked, n_double, n_float, first_bad, nullptr);
}

/* Build (or load from the cache file) the table of this process: every float in (0, 1] whose
 * device log2 differs from the host's, with the host's value.  About a second of work the first
 * time on a box; the list (some 12 MB) is then kept in a per-user cache directory -- $FIASCO_AMD_CACHE,
 * else $XDG_CACHE_HOME/fiasco_amd, else $HOME/.cache/fiasco_amd, /tmp only as the last resort -- under a
 * name that carries the host libm's and the device's answers to a few probe arguments.  A cache file is
 * taken only if its checksum fits and EVERY stored value is what this host's log2 computes now.
 *
 * log2_patch_build() returns false -- with the reason in err -- when the table is needed but could not be built or
 * brought onto the device: 1 018 853 arguments differ between ocml and glibc, frames coded without
 * the table could differ from the reference's streams, so fa_core_stage() fails them instead
 * (FIASCO_AMD_NO_LOG2_TABLE=1 runs without the table on purpose).  It is called by every staging call of every
 * thread: l2_once() (dev_state.h) lets ONE of them run log2_patch_fill() per share and device, the others wait for it
 * and leave with its answer -- a failure stays one, with the builder's reason, until the share meets another device. */

static unsigned long long fnv64(const void *p, size_t n, unsigned long long h = 1469598103934665603ull)
{
    const unsigned char *c = (const unsigned char *) p;
    for (size_t i = 0; i < n; i++) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}

static void mkdir_p(const char *dir)
{
    char tmp[512];
    snprintf(tmp, sizeof tmp, "%s", dir);
    for (char *q = tmp + 1; *q; q++)
        if (*q == '/') { *q = 0; (void) mkdir(tmp, 0700); *q = '/'; }
    (void) mkdir(tmp, 0700);
}

/* cache directory of this user; created if need be */
static void l2_cache_dir(char *out, size_t n)
{
    const char *e;
    if ((e = getenv("FIASCO_AMD_CACHE")) && *e) snprintf(out, n, "%s", e);
    else if ((e = getenv("XDG_CACHE_HOME")) && *e) snprintf(out, n, "%s/fiasco_amd", e);
    else if ((e = getenv("HOME")) && *e) snprintf(out, n, "%s/.cache/fiasco_amd", e);
    else snprintf(out, n, "/tmp");
    mkdir_p(out);
    if (access(out, W_OK) != 0) snprintf(out, n, "/tmp");
}

/* the builder's part (the share is in L2_BUILDING: nobody else reads or writes g_l2 and g_l2_err meanwhile) */
static bool log2_patch_fill(int dev)
{
    if (g_l2.d_keys) { (void) hipFree(g_l2.d_keys); (void) hipFree(g_l2.d_vals); }
    g_l2.d_keys = nullptr; g_l2.d_vals = nullptr; g_l2.mask = 0; g_l2.entries = 0;
    if (getenv("FIASCO_AMD_NO_LOG2_TABLE")) return true;
    if (fa_knob("FIASCO_AMD_FAIL_LOG2_TABLE")) {                    /* tests: what a failed build looks like */
        snprintf(g_l2_err, sizeof g_l2_err, "failure requested by FIASCO_AMD_FAIL_LOG2_TABLE");
        return false;
    }
    std::vector<std::pair<unsigned, double>> list;
    char path[600];
    {
        /* fingerprint: host libm on a few awkward arguments + device name */
        hipDeviceProp_t prop;
        unsigned long long fp = 1469598103934665603ull;
        const float probe[] = { 0.3f, 1.0f / 3, 0.7f, 5.0f / 7, 0.0123f, 0.999f, 1e-3f, 0.57f };
        for (unsigned i = 0; i < sizeof probe / sizeof probe[0]; i++) {
            double v = log2((double) probe[i]);
            unsigned long long b; memcpy(&b, &v, 8);
            fp = (fp ^ b) * 1099511628211ull;
        }
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess)
            for (const char *c = prop.gcnArchName; *c; c++) fp = (fp ^ (unsigned char) *c) * 1099511628211ull;
        int rt = 0; (void) hipRuntimeGetVersion(&rt);
        fp = (fp ^ (unsigned) rt) * 1099511628211ull;
        char dir[512];
        l2_cache_dir(dir, sizeof dir);
        snprintf(path, sizeof path, "%s/fiasco_amd_log2_%016llx.bin", dir, fp);
    }
    bool loaded = false;
    if (FILE *f = fopen(path, "rb")) {
        /* magic, entries, FNV-1a of the payload */
        unsigned long long hdr[3] = { 0, 0, 0 };
        if (fread(hdr, 8, 3, f) == 3 && hdr[0] == 0x33474f4c41464full && hdr[1] < (1ull << 26)) {
            list.resize((size_t) hdr[1]);
            loaded = fread(list.data(), sizeof list[0], list.size(), f) == list.size()
                     && fgetc(f) == EOF
                     && fnv64(list.data(), list.size() * sizeof list[0]) == hdr[2];
            /* every stored value must still be what this host computes (a second of log2 calls
             * at most: cheap next to trusting a file somebody else could have written) */
            for (size_t i = 0; loaded && i < list.size(); i++) {
                float pf; memcpy(&pf, &list[i].first, 4);
                double v = log2((double) pf);
                if (!(pf > 0.0f && pf <= 1.0f) || memcmp(&v, &list[i].second, 8) != 0) loaded = false;
            }
        }
        fclose(f);
        if (!loaded) list.clear();
    }
    if (!loaded) {
        unsigned long long nd = 0;
        if (!log2_compare(1, 127, false, nullptr, &nd, nullptr, nullptr, &list)) {
            snprintf(g_l2_err, sizeof g_l2_err, "the comparison of the device's log2 with the host's did not run (%s)",
                     hipGetErrorString(hipGetLastError()));
            return false;
        }
        char tmp[640];
        snprintf(tmp, sizeof tmp, "%s.%d", path, (int) getpid());
        int fd = open(tmp, O_WRONLY | O_CREAT | O_EXCL, 0600);
        if (FILE *f = fd >= 0 ? fdopen(fd, "wb") : nullptr) {
            unsigned long long hdr[3] = { 0x33474f4c41464full, (unsigned long long) list.size(),
                                          fnv64(list.data(), list.size() * sizeof list[0]) };
            bool ok = fwrite(hdr, 8, 3, f) == 3 && fwrite(list.data(), sizeof list[0], list.size(), f) == list.size();
            ok = fclose(f) == 0 && ok;
            if (!ok || rename(tmp, path) != 0) (void) remove(tmp);      /* no cache: built again next time */
        } else if (fd >= 0) close(fd);
    }
    g_l2.entries = list.size();
    if (list.empty()) return true;                           /* the two logarithms agree everywhere: nothing to correct */
    unsigned slots = 1024;
    while (slots < 4 * list.size()) slots <<= 1;
    std::vector<unsigned> keys(slots, 0u);
    std::vector<double> vals(slots, 0.0);
    for (size_t i = 0; i < list.size(); i++) {
        unsigned h = (list[i].first * 2654435761u) & (slots - 1);
        while (keys[h]) h = (h + 1) & (slots - 1);
        keys[h] = list[i].first; vals[h] = list[i].second;
    }
    hipError_t e;
    if ((e = hipMalloc((void **) &g_l2.d_keys, (size_t) slots * 4)) != hipSuccess
        || (e = hipMalloc((void **) &g_l2.d_vals, (size_t) slots * 8)) != hipSuccess
        || (e = hipMemcpy(g_l2.d_keys, keys.data(), (size_t) slots * 4, hipMemcpyHostToDevice)) != hipSuccess
        || (e = hipMemcpy(g_l2.d_vals, vals.data(), (size_t) slots * 8, hipMemcpyHostToDevice)) != hipSuccess) {
        (void) hipGetLastError();
        if (g_l2.d_keys) (void) hipFree(g_l2.d_keys);
        if (g_l2.d_vals) (void) hipFree(g_l2.d_vals);
        g_l2.d_keys = nullptr; g_l2.d_vals = nullptr;
        snprintf(g_l2_err, sizeof g_l2_err, "%llu corrections could not be brought onto the device (%s)",
                 (unsigned long long) list.size(), hipGetErrorString(e));
        return false;
    }
    g_l2.mask = slots - 1;
    return true;
}

static bool log2_patch_build(char *err, size_t n)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void) hipGetLastError(); snprintf(err, n, "no current HIP device"); return false; }
    return l2_once(t_dev, dev, [dev] { return log2_patch_fill(dev); }, err, n);
}

/* the same comparison THROUGH the table the frame kernel uses: n_double must come out 0 */
extern "C" int fiasco_amd_selftest_log2_patched(unsigned exp_lo, unsigned exp_hi, unsigned long long *n_checked,
                                                unsigned long long *n_double, unsigned long long *n_entries)
{
    char why[200];
    if (!log2_patch_build(why, sizeof why)) { fa_set_error("selftest: no log2 table on this device: %s", why); return 0; }
    if (n_entries) *n_entries = g_l2.entries;
    if (!g_l2.d_keys && g_l2.entries) { fa_set_error("selftest: no log2 table on this device"); return 0; }
    return log2_compare(exp_lo, exp_hi, g_l2.d_keys != nullptr, n_checked, n_double, nullptr, nullptr, nullptr);
}
