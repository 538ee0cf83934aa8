// ek_pam_limits.h -- the sizes of the PAM window path that kernels (ek_common.h,
// ek_pam_sparse.h) and the host's policy (ek_pam_policy.h) both read.  Plain numbers:
// nothing of HIP.
#pragma once

// PAM: proposals per prefetch pass / columns per workgroup of the pairs kernel
#define EK_PAM_GROUP 8
// a window of proposals decided on the device (ek_pam_window_run): up to
// EK_PAM_WIN consecutive clusters, their proposals drawn, prefetched (in groups
// of EK_PAM_GROUP columns) and decided without a host round trip in between
#ifndef EK_PAM_WIN
#define EK_PAM_WIN 32     // (16 in round 2: the set-up of a window is ~240 us whatever its width)
#endif
static_assert(EK_PAM_WIN % EK_PAM_GROUP == 0 && EK_PAM_WIN <= 32,
              "whole column groups; the stale mask is 32 bits");
// numpy's summation order (ek_pam.hip, "cost sums in numpy's order")
#define EK_PW_FULL_LEAVES 64        // leaves of a full chunk (128 elements each)
// frames on a window's list (ek_pam_active_kernel) up to which the one-workgroup
// form is used; above it the three launches per proposal of ek_pam.hip are
#define EK_SP_CAP 65536
// (ambiguous member, medoid within reach) pairs one workgroup searches itself;
// a proposal with more ends the window and goes through the launches
#define EK_SP_MAX_PAIRS 16384
// chunks of 8192 frames whose sums the workgroup keeps in LDS (shards of up to
// 8.4 million frames)
#define EK_SP_MAX_CHUNKS 1024
