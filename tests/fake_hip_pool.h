/*
 *  fake_hip_pool.h -- the five HIP calls of csrc/hip/slab_pool.inc over malloc and free, for tests/dev_state_check.cpp.
 *
 *  hipMalloc / hipFree are malloc / free under a settable byte budget, hipMemGetInfo reports what is left of it (on
 *  top of the reserve slab_acquire keeps free), hipGetDevice answers a per-thread value, hipGetLastError is empty.
 *  The fake takes no lock of its own -- its books are atomics -- so that it orders nothing between two threads of the
 *  code under test: a race in the pool stays one for the thread sanitizer.  Every allocation carries a header that says
 *  whether it is live: a second free of the same block is counted (and is a use after free for the address sanitizer).
 */
#ifndef FAKE_HIP_POOL_H
#define FAKE_HIP_POOL_H 1
#include <atomic>
#include <new>
#include <stddef.h>
#include <stdlib.h>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };

namespace fake_hip {
enum : unsigned long long { LIVE = 0x6c6976656c697665ull, DEAD = 0x6465616464656164ull };
struct Header { std::atomic<unsigned long long> tag; size_t bytes; };
enum { HEADER = 64 };                                   /* keeps what hipMalloc returns aligned */
static const size_t RESERVE = (size_t) 768 << 20;       /* what slab_acquire leaves free on a real device */
static std::atomic<size_t> budget(0), used(0);
static std::atomic<unsigned long long> mallocs(0), refused(0), frees(0), bad_frees(0);
static thread_local int device = 0;
}

static hipError_t hipGetDevice(int *d) { *d = fake_hip::device; return hipSuccess; }
static hipError_t hipGetLastError(void) { return hipSuccess; }

static hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b)
{
    const size_t b = fake_hip::budget.load(), u = fake_hip::used.load();
    *total_b = b + fake_hip::RESERVE;
    *free_b = (b > u ? b - u : 0) + fake_hip::RESERVE;
    return hipSuccess;
}

static hipError_t hipMalloc(void **p, size_t bytes)
{
    using namespace fake_hip;
    *p = nullptr;
    if (used.fetch_add(bytes) + bytes > budget.load()) { used.fetch_sub(bytes); refused++; return hipErrorOutOfMemory; }
    char *raw = (char *) malloc(HEADER + bytes);
    if (!raw) { used.fetch_sub(bytes); refused++; return hipErrorOutOfMemory; }
    Header *h = new (raw) Header;
    h->tag.store(LIVE); h->bytes = bytes;
    mallocs++;
    *p = raw + HEADER;
    return hipSuccess;
}

static hipError_t hipFree(void *p)
{
    using namespace fake_hip;
    if (!p) return hipSuccess;
    Header *h = (Header *) ((char *) p - HEADER);
    if (h->tag.exchange(DEAD) != LIVE) { bad_frees++; return hipErrorInvalidValue; }     /* freed twice, or never allocated */
    used.fetch_sub(h->bytes);
    frees++;
    free(h);
    return hipSuccess;
}

#endif
