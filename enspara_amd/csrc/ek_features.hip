// ek_features.hip -- point-vs-set distances in feature space.
//
// Replaces the reference's only native distance code, the Cython/OpenMP
// kernels of enspara/geometry/libdist.pyx (bound as metrics 'euclidean' and
// 'manhattan'/'cityblock' at enspara/cluster/util.py:292-295):
//   _euclidean :122-145   out[i] = sqrt( sum_j (X[i,j] - y[j])**2 )
//   _manhattan :100-117   out[i] = sum_j fabs(X[i,j] - y[j])
//   _hamming   :77-95     out[i] = (number of j with X[i,j] != y[j]) / n_features
// Output is float64 in all three.  Arithmetic contract (what the generated C
// of the reference does, so results are bit-identical):
//   float32 input: the difference and its square are float32 operations, the
//   running sum is float64, terms added in feature order; manhattan widens the
//   float32 difference to float64 before fabs;
//   float64 input: everything in float64;
//   hamming: exact integer comparison.
//
// Same mapping as the RMSD kernels: samples are stored feature-major in tiles
// of 256 ("frame-minor"), one lane owns one sample and walks the features in
// order (no cross-lane reduction, order fixed), the target point is staged in
// LDS in chunks and read as wave-wide broadcasts.  HBM-bound: 4 or 8 bytes per
// (sample, feature) and ~2 flops.
#include "ek_feat.h"

#include <algorithm>
#include <new>

// ---- row-major [count][F] -> tiles, through LDS -------------------------------
template <typename T>
__global__ void __launch_bounds__(EK_BLOCK)
feat_transpose_kernel(const T *__restrict__ src, int64_t count, int F,
                      T *__restrict__ tiles, int64_t first)
{
    __shared__ T stage[EK_BLOCK * (FT_CHUNK + 1)];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * EK_BLOCK;
    const int64_t rows = (count - r0 < EK_BLOCK) ? (count - r0) : EK_BLOCK;
    const int64_t g = first + r0 + t;
    T *obase = feat_tile_ptr(tiles, g, F);
    for (int j0 = 0; j0 < F; j0 += FT_CHUNK) {
        const int w = (F - j0 < FT_CHUNK) ? (F - j0) : FT_CHUNK;
        const int64_t total = rows * w;
        for (int64_t i = t; i < total; i += EK_BLOCK) {
            const int r = (int)(i / w), j = (int)(i % w);
            stage[r * (FT_CHUNK + 1) + j] = src[(size_t)(r0 + r) * F + j0 + j];
        }
        __syncthreads();
        if (t < rows)
            for (int j = 0; j < w; ++j)
                obase[(size_t)(j0 + j) * EK_TILE] = stage[t * (FT_CHUNK + 1) + j];
        __syncthreads();
    }
}

// ---- distances -----------------------------------------------------------------
template <typename T, int METRIC>
__global__ void __launch_bounds__(EK_BLOCK)
feat_distance_kernel(const T *__restrict__ tiles, const T *__restrict__ y,
                     int64_t n, int F, double *__restrict__ out)
{
    __shared__ T ys[FY_CHUNK];
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    const double acc = feat_one_vs_all<T, METRIC>(feat_tile_ptr(tiles, f, F), y, F, ys);
    if (f < n)
        out[f] = feat_finish<METRIC>(acc, F);
}

// out[i] = metric(sample i, y), both on the device
void feat_enqueue_distance(ek_feat *k, int32_t metric)
{
    const unsigned blocks = (unsigned)((k->n + EK_BLOCK - 1) / EK_BLOCK);
    feat_dispatch(k, metric, [&](auto t, auto m) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((feat_distance_kernel<T, decltype(m)::value>), dim3(blocks),
                           dim3(EK_BLOCK), 0, k->s, (const T *)k->tiles, (const T *)k->y,
                           k->n, k->F, k->out);
    });
}

// ---- C ABI ----------------------------------------------------------------------
extern "C" int ek_feat_destroy(ek_feat *k)
{
    if (!k)
        return EK_OK;
    ek_feat_pam_release(k);
    (void)hipSetDevice(k->device);
    if (k->s)
        (void)hipStreamSynchronize(k->s);
    (void)ek_dev_free(k->tiles);
    (void)ek_dev_free(k->stage);
    (void)ek_dev_free(k->y);
    (void)ek_dev_free(k->out);
    (void)ek_dev_free(k->kdist);
    (void)ek_dev_free(k->kassign);
    (void)ek_dev_free(k->bm);
    (void)ek_dev_free(k->ctl);
    (void)ek_dev_free(k->hist);
    (void)ek_dev_free(k->sctl);
    (void)ek_dev_free(k->shist_idx);
    (void)ek_dev_free(k->shist_d);
    (void)ek_dev_free(k->acent);
    (void)ek_dev_free(k->apart_d);
    (void)ek_dev_free(k->apart_c);
    if (k->s && k->own_stream)
        (void)ek_stream_destroy(k->s);
    delete k;
    return EK_OK;
}

// (global_offset, stream: a shard of a larger sample set on the caller's stream;
// stream == NULL: a stream of the handle's own)
extern "C" int ek_feat_create_sharded(int device, int64_t n_samples,
                                      int32_t n_features, int32_t elem_kind,
                                      int64_t global_offset, void *stream,
                                      ek_feat **out)
{
    if (!out || n_samples < 0 || n_features < 1 || elem_kind < 0 ||
        elem_kind > 2 || global_offset < 0)
        return ek_set_error(EK_EARG, "ek_feat_create: bad argument");
    *out = nullptr;
    FE_HIP(hipSetDevice(device));
    ek_feat *k = new (std::nothrow) ek_feat();
    if (!k)
        return ek_set_error(EK_ENOMEM, "ek_feat_create: out of memory");
    k->device = device;
    k->n = n_samples;
    k->F = n_features;
    k->kind = elem_kind;
    k->esize = elem_kind == 0 ? 4 : 8;
    k->n_tiles = (n_samples + EK_TILE - 1) / EK_TILE;
    k->goff = global_offset;
    const size_t tb = (size_t)std::max<int64_t>(k->n_tiles, 1) * n_features *
                      EK_TILE * k->esize;
    hipError_t e = hipSuccess;
    if (stream) {
        k->s = (hipStream_t)stream;
        k->own_stream = false;
    } else {
        e = ek_stream_create_flags(&k->s, hipStreamNonBlocking);
    }
    if (e == hipSuccess)
        e = ek_dev_malloc(&k->tiles, tb);
    if (e == hipSuccess)
        e = hipMemsetAsync(k->tiles, 0, tb, k->s);
    if (e == hipSuccess)
        e = ek_dev_malloc(&k->y, (size_t)n_features * k->esize);
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&k->out,
                      (size_t)std::max<int64_t>(n_samples, 1) * sizeof(double));
    if (e != hipSuccess) {
        ek_feat_destroy(k);
        return ek_set_error(e == hipErrorOutOfMemory ? EK_ENOMEM : EK_EHIP,
                            "ek_feat_create: %s", hipGetErrorString(e));
    }
    *out = k;
    return EK_OK;
}

extern "C" int ek_feat_create(int device, int64_t n_samples, int32_t n_features,
                              int32_t elem_kind, ek_feat **out)
{
    return ek_feat_create_sharded(device, n_samples, n_features, elem_kind, 0,
                                  nullptr, out);
}

extern "C" int ek_feat_load(ek_feat *k, const void *X, int64_t first,
                            int64_t count)
{
    if (!k || (!X && count > 0) || first < 0 || count < 0 ||
        first + count > k->n || first % EK_TILE)
        return ek_set_error(EK_EARG, "ek_feat_load: bad argument");
    FE_HIP(hipSetDevice(k->device));
    const size_t row = (size_t)k->F * k->esize;
    int64_t chunk = (int64_t)((128u << 20) / row);
    chunk = std::max<int64_t>(EK_TILE, chunk / EK_TILE * EK_TILE);
    chunk = std::min<int64_t>(chunk, (count + EK_TILE - 1) / EK_TILE * EK_TILE);
    if (chunk > k->stage_rows) {
        FE_HIP(hipStreamSynchronize(k->s));
        (void)ek_dev_free(k->stage);
        k->stage = nullptr;
        k->stage_rows = 0;
        FE_HIP(ek_dev_malloc(&k->stage, (size_t)chunk * row));
        k->stage_rows = chunk;
    }
    for (int64_t done = 0; done < count; done += chunk) {
        const int64_t cnt = std::min(chunk, count - done);
        FE_HIP(hipMemcpyAsync(k->stage, (const char *)X + (size_t)done * row,
                              (size_t)cnt * row, hipMemcpyHostToDevice, k->s));
        const unsigned blocks = (unsigned)((cnt + EK_BLOCK - 1) / EK_BLOCK);
        feat_dispatch_size(k, [&](auto t) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL(feat_transpose_kernel<T>, dim3(blocks), dim3(EK_BLOCK), 0,
                               k->s, (const T *)k->stage, cnt, k->F, (T *)k->tiles,
                               first + done);
        });
        FE_HIP(hipGetLastError());
        FE_HIP(hipStreamSynchronize(k->s));
    }
    k->loaded = true;
    return EK_OK;
}

extern "C" int ek_feat_distance(ek_feat *k, int32_t metric, const void *y,
                                double *out_host)
{
    if (!k || !y || !out_host || metric < 0 || metric > 2)
        return ek_set_error(EK_EARG, "ek_feat_distance: bad argument");
    if (!k->loaded)
        return ek_set_error(EK_ESTATE, "ek_feat_distance: no samples loaded");
    if (int rc = feat_metric_ok(k, metric, "ek_feat_distance"))
        return rc;
    if (k->n == 0)
        return EK_OK;
    FE_HIP(hipSetDevice(k->device));
    FE_HIP(hipMemcpyAsync(k->y, y, (size_t)k->F * k->esize,
                          hipMemcpyHostToDevice, k->s));
    feat_enqueue_distance(k, metric);
    FE_HIP(hipGetLastError());
    FE_HIP(hipMemcpyAsync(out_host, k->out, (size_t)k->n * sizeof(double),
                          hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipStreamSynchronize(k->s));
    return EK_OK;
}
