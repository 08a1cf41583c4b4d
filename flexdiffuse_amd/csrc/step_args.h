// The argument rules that the step fronts of step.hip, window.hip and composite.hip share, each written once.  Host code only:
// nothing here is compiled for the device.
#pragma once
#include "common.h"

#define FD_TRY(call)                   \
    do {                               \
        const int rc_ = (call);        \
        if (rc_ != FD_OK) return rc_;  \
    } while (0)

// B, C, HW positive; the NHWC eps rows (where the call has any) at least C wide
static inline int fd_step_sizes(const char* who, int B, int C, int HW, int ld, bool rows) {
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && (!rows || ld >= C), FD_EINVAL, "%s: sizes", who);
    return FD_OK;
}

// the known-region blend: a mask needs z0 and noise, and neither may be the buffer `x` the step updates in place (`what`)
static inline int fd_blend_args(const char* who, const void* x, const void* z0, const void* nz, const void* mask,
                                const char* what) {
    FD_CHECK_ARG(!mask || (z0 && nz), FD_EINVAL, "%s: mask without z0 / noise (null)", who);
    FD_CHECK_ARG(!mask || (x != z0 && x != nz), FD_EINVAL, "%s: z0 / noise alias the %s", who, what);
    return FD_OK;
}

// composition: eps_nhwc holds (cfg + 1 + n_entities) B HW rows, weights fp32 [n_entities][HW]
static inline int fd_entity_args(const char* who, const void* weights, int n_entities) {
    FD_CHECK_ARG(n_entities >= 0, FD_EINVAL, "%s: n_entities %d is negative", who, n_entities);
    FD_CHECK_ARG(n_entities == 0 || weights, FD_EINVAL, "%s: weights are null with n_entities %d", who, n_entities);
    return FD_OK;
}
