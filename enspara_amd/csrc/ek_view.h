// ek_view.h -- the active view of a shard (ek_view.hip): the frames a k-centers round
// can still change, compacted in ascending order into a second, smaller frame store.
// Host side declarations only; the distance kernels know nothing of it.
#pragma once
#include "ek_common.h"

#define EK_VIEW_SEL 1024    // frames per workgroup of the select kernels

// scratch of a selection: per-workgroup counts and their exclusive scan
static inline size_t ek_view_sel_blocks(int64_t n)
{
    return (size_t)((n + EK_VIEW_SEL - 1) / EK_VIEW_SEL);
}
// count[0] = frames of dist[0 .. n) with dist > theta (NaN counts: it is not settled);
// with act != nullptr also act[p] = their positions, ascending, for p < act_cap.
// blockcnt / blockoff: ek_view_sel_blocks(n) entries each (blockoff only with act).
void ek_launch_view_select(const float *dist, int64_t n, float theta, uint32_t *blockcnt,
                           uint32_t *blockoff, uint32_t *act, int64_t act_cap,
                           uint32_t *count, hipStream_t s);
// the view's store from the shard's: bit copies of the centred frames (frame-minor
// tiles), traces, distances and labels of frames act[0 .. n_v); the slots of padding of
// the last tile are zeros.  A view has no frame-major copy: ek_round_row (ek_common.h)
void ek_launch_view_gather(const uint32_t *act, int64_t n_v, int A, const float *aos,
                           const double *G, const float *dist, const int32_t *assign,
                           float *tiles_v, double *G_v, float *dist_v, int32_t *assign_v,
                           hipStream_t s);
// the gather of a rebuild: as ek_launch_view_gather, but out_v is the view's QUAD copy
// (quad: the layout of ek_launch_quad_tiles, whole tiles, zeros for the atoms past the
// last and the frames of padding) or its frame-minor tiles (!quad)
void ek_launch_view_build(const uint32_t *act, int64_t n_v, int A, bool quad, const float *aos,
                          const double *G, const float *dist, const int32_t *assign,
                          float *out_v, double *G_v, float *dist_v, int32_t *assign_v,
                          hipStream_t s);
// frame-minor tiles from a quad copy (the inverse of ek_launch_quad_tiles), bit copies
void ek_launch_view_tiles(const float *qtiles, int64_t n_tiles, int A, float *tiles,
                          hipStream_t s);
// One launch: count[2 parity] += frames of dist[0 .. n) above theta, count[2 parity + 1] +=
// frames of shard_dist[0 .. shard_n) above it (shard_dist may be null: no view), where
// theta is what the host derives from ctl->last_max: (rho last_max - abs) / (2 (1 + rel))
// in double, rounded down; the other parity's two words are set to zero.  count: four
// words, the two of `parity` zero on entry -- the looks of a context alternate, and the
// host has read a look's words before it enqueues the next
void ek_launch_view_look(const float *dist, int64_t n, const float *shard_dist,
                         int64_t shard_n, const EkCtl *ctl, double rho, double rel,
                         double abs_, uint32_t *count, int parity, hipStream_t s);
// count[0] += 32-bit words of a[0 .. words) and b[0 .. words) that differ
void ek_launch_view_diff(const void *a, const void *b, size_t words,
                         unsigned long long *count, hipStream_t s);
// dist[act[p]] = dist_v[p], assign[act[p]] = assign_v[p]; the centers accepted under
// the view (labels label_lo .. n_done - 1, n_done read from ctl) get their positions in
// the shard: hist[l].gidx = goff + act[hist[l].gidx - goff]
void ek_launch_view_scatter(const uint32_t *act, int64_t n_v, const float *dist_v,
                            const int32_t *assign_v, float *dist, int32_t *assign,
                            EkHist *hist, int32_t label_lo, int32_t label_cap,
                            const EkCtl *ctl, int64_t goff, hipStream_t s);
