// ek_mi_launch.h -- the pack, count and information kernels of ek_mi.hip as launch
// functions, so that ek_cards.hip counts its resident codes with the same kernels.
// All of them only enqueue on `s`; the caller checks hipGetLastError and synchronises.
#pragma once
#include "ek_common.h"

#define MI_CHUNK 16384          // frames of a workgroup (enspara_amd.info_theory.MI_CHUNK)
#define MI_PAD 255              // the code of a padding frame: no state (n <= 255)
#define MI_MAX_STATES 255
#define MI_MAX_GRID_Z 65535
#define MI_MAX_FEATURES (MI_MAX_GRID_Z * 64)   // the pack kernel takes 64 features per grid.y
#define MI_BLOCK 128            // rows / columns of a workgroup: 2 x 2 waves

// frames padded to the 64 of one MFMA step
static inline int64_t ek_mi_tpad(int64_t frames) { return (frames + 63) / 64 * 64; }

// in [frames][F] uint8 -> out [F][tpad], MI_PAD behind the last frame
void ek_mi_launch_pack(const uint8_t *in, int64_t frames, int32_t F, int64_t tpad, uint8_t *out,
                       hipStream_t s);
// jc [fx][fy][nx][ny] += the joint counts of cx [fx][tpad] against cy [fy][tpad]
void ek_mi_launch_count(const uint8_t *cx, const uint8_t *cy, int64_t tpad, int32_t fx,
                        int32_t fy, int32_t nx, int32_t ny, uint32_t *jc, hipStream_t s);
// mi [pairs] from jc [pairs][nx][ny]; col [pairs][ny] uint32 scratch
void ek_mi_launch_info(const uint32_t *jc, int64_t pairs, int32_t nx, int32_t ny, uint32_t *col,
                       double *mi, hipStream_t s);
// EK_ENOMEM (with the message) unless `bytes` and some slack are free on the current device
int ek_mi_check_memory(size_t bytes, const char *who);
// the limits ek_mi_open puts on features x states of one side of the count kernel's grid
int ek_mi_check_shape(int32_t fx, int32_t fy, int32_t nx, int32_t ny, const char *who);
