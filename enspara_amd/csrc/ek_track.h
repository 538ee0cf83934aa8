// ek_track.h -- the counted front for device resources.
//
// Every device allocation, pinned host allocation, stream and event of the library
// is made and released through these functions; the raw HIP calls occur in
// ek_track.hip only (tests/test_track_host.py holds the sources to that).  The
// counts are what ek_live_resources reports and what tests/test_gpu_lifetime.py
// balances; ek_fail_alloc_at makes one device allocation fail without touching the
// device.  None of this sits inside a timed loop: the run loops allocate nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

hipError_t ek_dev_malloc_raw(void **ptr, size_t bytes);
// device memory with allocation flags (the uncached mailboxes of ek_api.hip)
hipError_t ek_dev_malloc_flags_raw(void **ptr, size_t bytes, unsigned int flags);
hipError_t ek_dev_free(void *ptr);
hipError_t ek_pinned_malloc_raw(void **ptr, size_t bytes, unsigned int flags);
hipError_t ek_pinned_free(void *ptr);
hipError_t ek_stream_create_flags(hipStream_t *s, unsigned int flags);
hipError_t ek_stream_destroy(hipStream_t s);
hipError_t ek_event_create(hipEvent_t *e);
hipError_t ek_event_create_flags(hipEvent_t *e, unsigned int flags);
hipError_t ek_event_destroy(hipEvent_t e);

// typed pointers, as the HIP runtime's own templates take them
template <class T>
static inline hipError_t ek_dev_malloc(T **ptr, size_t bytes)
{
    return ek_dev_malloc_raw((void **)ptr, bytes);
}
template <class T>
static inline hipError_t ek_dev_malloc_flags(T **ptr, size_t bytes, unsigned int flags)
{
    return ek_dev_malloc_flags_raw((void **)ptr, bytes, flags);
}
template <class T>
static inline hipError_t ek_pinned_malloc(T **ptr, size_t bytes,
                                          unsigned int flags = hipHostMallocDefault)
{
    return ek_pinned_malloc_raw((void **)ptr, bytes, flags);
}
