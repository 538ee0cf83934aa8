// ek_track.hip -- the counted front for device resources (ek_track.h): the one
// file of csrc/ that calls hipMalloc, hipExtMallocWithFlags, hipFree, hipHostMalloc,
// hipHostFree, hipStreamCreateWithFlags, hipStreamDestroy, hipEventCreate[WithFlags]
// and hipEventDestroy.
//
// The counters are atomics (the upload path has copy threads); the sizes of live
// blocks sit in two maps behind one mutex, which also orders the armed failure
// among concurrent allocations.  An allocation costs a map insert on top of the
// runtime's own work -- nothing next to hipMalloc, and no run loop allocates.
#include "ek_track.h"
#include "../../include/enspara_hip.h"
#include <atomic>
#include <mutex>
#include <unordered_map>

namespace {
std::atomic<int64_t> g_dev_n{0}, g_dev_bytes{0}, g_pin_n{0}, g_pin_bytes{0};
std::atomic<int64_t> g_streams{0}, g_events{0}, g_dev_total{0};
std::atomic<int64_t> g_fail_at{-1};
std::mutex g_mutex;
// (leaked on purpose: a handle closed by a static destructor of another library
// after this file's statics are gone must still find them)
std::unordered_map<void *, size_t> &dev_blocks()
{
    static auto *m = new std::unordered_map<void *, size_t>();
    return *m;
}
std::unordered_map<void *, size_t> &pin_blocks()
{
    static auto *m = new std::unordered_map<void *, size_t>();
    return *m;
}

// the armed failure: true = this allocation is the one that fails
bool take_failure()
{
    std::lock_guard<std::mutex> lock(g_mutex);
    const int64_t k = g_fail_at.load(std::memory_order_relaxed);
    if (k < 0)
        return false;
    g_fail_at.store(k - 1, std::memory_order_relaxed);     // (0 -> -1: clear)
    return k == 0;
}

// No HIP call is made with the mutex held (a release waits for the device, and the
// device may be waiting for a kernel another thread has yet to launch).  A block is
// entered after the runtime handed it out and struck off BEFORE it is given back, so
// an address that goes from one thread's release to another's allocation is never
// struck off after it was entered again.
void enter(std::unordered_map<void *, size_t> &blocks, std::atomic<int64_t> &n,
           std::atomic<int64_t> &bytes_live, void *ptr, size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    blocks[ptr] = bytes;
    n.fetch_add(1, std::memory_order_relaxed);
    bytes_live.fetch_add((int64_t)bytes, std::memory_order_relaxed);
}
// -> the block's size, or -1 if it is not one of ours
int64_t strike(std::unordered_map<void *, size_t> &blocks, std::atomic<int64_t> &n,
               std::atomic<int64_t> &bytes_live, void *ptr)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = blocks.find(ptr);
    if (it == blocks.end())
        return -1;
    const int64_t bytes = (int64_t)it->second;
    blocks.erase(it);
    n.fetch_sub(1, std::memory_order_relaxed);
    bytes_live.fetch_sub(bytes, std::memory_order_relaxed);
    return bytes;
}

template <class F>
hipError_t dev_alloc(void **ptr, size_t bytes, F &&call)
{
    if (take_failure()) {
        if (ptr)
            *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    const hipError_t e = call();
    if (e == hipSuccess && ptr && *ptr) {
        enter(dev_blocks(), g_dev_n, g_dev_bytes, *ptr, bytes);
        g_dev_total.fetch_add(1, std::memory_order_relaxed);
    }
    return e;
}
}   // namespace

hipError_t ek_dev_malloc_raw(void **ptr, size_t bytes)
{
    return dev_alloc(ptr, bytes, [&] { return hipMalloc(ptr, bytes); });
}

hipError_t ek_dev_malloc_flags_raw(void **ptr, size_t bytes, unsigned int flags)
{
    return dev_alloc(ptr, bytes, [&] { return hipExtMallocWithFlags(ptr, bytes, flags); });
}

hipError_t ek_dev_free(void *ptr)
{
    if (!ptr)
        return hipSuccess;
    const int64_t bytes = strike(dev_blocks(), g_dev_n, g_dev_bytes, ptr);
    const hipError_t e = hipFree(ptr);
    if (e != hipSuccess && bytes >= 0)      // (still there: it counts again)
        enter(dev_blocks(), g_dev_n, g_dev_bytes, ptr, (size_t)bytes);
    return e;
}

hipError_t ek_pinned_malloc_raw(void **ptr, size_t bytes, unsigned int flags)
{
    const hipError_t e = hipHostMalloc(ptr, bytes, flags);
    if (e == hipSuccess && ptr && *ptr)
        enter(pin_blocks(), g_pin_n, g_pin_bytes, *ptr, bytes);
    return e;
}

hipError_t ek_pinned_free(void *ptr)
{
    if (!ptr)
        return hipSuccess;
    const int64_t bytes = strike(pin_blocks(), g_pin_n, g_pin_bytes, ptr);
    const hipError_t e = hipHostFree(ptr);
    if (e != hipSuccess && bytes >= 0)
        enter(pin_blocks(), g_pin_n, g_pin_bytes, ptr, (size_t)bytes);
    return e;
}

hipError_t ek_stream_create_flags(hipStream_t *s, unsigned int flags)
{
    const hipError_t e = hipStreamCreateWithFlags(s, flags);
    if (e == hipSuccess)
        g_streams.fetch_add(1, std::memory_order_relaxed);
    return e;
}

hipError_t ek_stream_destroy(hipStream_t s)
{
    const hipError_t e = hipStreamDestroy(s);
    if (e == hipSuccess)
        g_streams.fetch_sub(1, std::memory_order_relaxed);
    return e;
}

hipError_t ek_event_create(hipEvent_t *ev)
{
    const hipError_t e = hipEventCreate(ev);
    if (e == hipSuccess)
        g_events.fetch_add(1, std::memory_order_relaxed);
    return e;
}

hipError_t ek_event_create_flags(hipEvent_t *ev, unsigned int flags)
{
    const hipError_t e = hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess)
        g_events.fetch_add(1, std::memory_order_relaxed);
    return e;
}

hipError_t ek_event_destroy(hipEvent_t ev)
{
    const hipError_t e = hipEventDestroy(ev);
    if (e == hipSuccess)
        g_events.fetch_sub(1, std::memory_order_relaxed);
    return e;
}

extern "C" int ek_live_resources(int64_t *out)
{
    if (!out)
        return EK_EARG;
    out[0] = g_dev_n.load();
    out[1] = g_dev_bytes.load();
    out[2] = g_pin_n.load();
    out[3] = g_pin_bytes.load();
    out[4] = g_streams.load();
    out[5] = g_events.load();
    out[6] = g_dev_total.load();
    return EK_OK;
}

extern "C" int64_t ek_fail_alloc_at(int64_t k)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    const int64_t was = g_fail_at.load();
    g_fail_at.store(k < 0 ? -1 : k);
    return was < 0 ? -1 : was;
}
