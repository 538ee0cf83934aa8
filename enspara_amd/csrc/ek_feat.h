// ek_feat.h -- what the feature-space sources share (ek_features.hip,
// ek_feat_assign.hip): the handle, and the arithmetic of one (sample, point)
// distance -- FeatAcc's chain over the features in order, then feat_finish.
#pragma once
#include "ek_common.h"

extern int ek_set_error(int code, const char *fmt, ...);

#define FT_CHUNK 32           // features per staged transposition chunk
#define FY_CHUNK 2048         // target-point features staged in LDS at a time

struct FeatPam;           // working set of ek_feat_pam_sweep (ek_features.hip)

struct ek_feat {
    int device = 0;
    int64_t n = 0;
    int32_t F = 0;
    int32_t kind = 0;         // 0 float32, 1 float64, 2 int64
    int32_t esize = 4;
    int64_t n_tiles = 0;
    hipStream_t s = nullptr;
    void *tiles = nullptr;    // [n_tiles][F][EK_TILE] elements
    void *stage = nullptr;
    int64_t stage_rows = 0;
    void *y = nullptr;        // [F] elements
    double *out = nullptr;    // [n]
    bool loaded = false;
    // device-resident k-centers state (ek_feat_kcenters)
    double *kdist = nullptr;  // [n] float64, as the reference keeps it
    int32_t *kassign = nullptr;
    struct FeatBlockMax *bm = nullptr;
    struct FeatCtl *ctl = nullptr;
    int64_t *hist = nullptr;
    int32_t hist_cap = 0;
    FeatPam *pam = nullptr;
    // one shard of a k-centers run over several handles (ek_feat_kcenters_step)
    bool own_stream = true;   // false: s is the caller's (ek_feat_create_sharded)
    int64_t goff = 0;         // global index of local sample 0
    struct FeatShardCtl *sctl = nullptr;
    int64_t *shist_idx = nullptr;   // [shist_cap] winners' global indices
    double *shist_d = nullptr;      // ... and their distances before the update
    int32_t shist_cap = 0;
    // ek_feat_assign_nearest (ek_feat_assign.hip): the center table and, where the
    // centers are split over workgroups, each part's nearest per sample
    void *acent = nullptr;          // [acent_cap] bytes
    size_t acent_cap = 0;
    double *apart_d = nullptr;      // [apart_cap] (part, sample)
    int32_t *apart_c = nullptr;
    size_t apart_cap = 0;
};

// the state arrays (kdist / kassign and what the sharded steps keep beside them)
int feat_shard_alloc(ek_feat *k, int32_t label);

#define FE_HIP(call)                                                           \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess)                                                  \
            return ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,      \
                                hipGetErrorString(e_), __FILE__, __LINE__);    \
    } while (0)

template <typename T, int METRIC> struct FeatAcc;
// euclidean
template <> struct FeatAcc<float, 0> {
    static __device__ __forceinline__ void add(double &acc, float x, float y)
    {
        const float d = x - y;           // float32 subtraction
        const float q = d * d;           // float32 product (powf(d, 2) == d*d)
        acc = acc + (double)q;
    }
};
template <> struct FeatAcc<double, 0> {
    static __device__ __forceinline__ void add(double &acc, double x, double y)
    {
        const double d = x - y;
        acc = acc + d * d;
    }
};
// manhattan
template <> struct FeatAcc<float, 1> {
    static __device__ __forceinline__ void add(double &acc, float x, float y)
    {
        const float d = x - y;
        acc = acc + __builtin_fabs((double)d);
    }
};
template <> struct FeatAcc<double, 1> {
    static __device__ __forceinline__ void add(double &acc, double x, double y)
    {
        acc = acc + __builtin_fabs(x - y);
    }
};
// hamming
template <> struct FeatAcc<long long, 2> {
    static __device__ __forceinline__ void add(double &acc, long long x,
                                               long long y)
    {
        if (x != y)
            acc = acc + 1.0;
    }
};

// what libdist.pyx does with a row's sum: sqrt (:143), nothing (:119), / n_features (:93)
template <int METRIC> __device__ __forceinline__ double feat_finish(double acc, int F)
{
    if (METRIC == 0)
        return __builtin_sqrt(acc);
    if (METRIC == 2)
        return acc / (double)F;
    return acc;
}
