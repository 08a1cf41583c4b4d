// The counter-based normal stream of the stochastic samplers, stated ONCE: k_latent_step's noise stage (step.hip:
// fd_cfg_ddim_noise_step_f32, fd_cfg_multistep_noise_step_f32) and the stand-alone fill (fd_philox_normal_f32) call
// these, so a value is a pure function of its address (seed, sample, element, draw, stream) and never of the kernel,
// the vector width, the batch split or the (B, C) view that asked for it.
//   generator  Philox4x32-10 (Salmon et al. 2011, "Parallel Random Numbers: As Easy as 1, 2, 3"), plain integer C++
//   key        (seed & 0xffffffff, seed >> 32)
//   counter    (q, sample, draw, stream): q = (element inside its sample) >> 2, sample = sample_offset + flat / per
//   words      w0..w3 of one counter -> the normals of elements 4q..4q+3; lanes (0, 1) from (w0, w1), (2, 3) from (w2, w3)
//   transform  u = ((wa >> 8) + 1) 2^-24 in (0, 1], f = (wb >> 8) 2^-23 in [0, 2) (both exact in fp32),
//              r = sqrt(-2 log u), z_even = r cospi(f), z_odd = r sinpi(f); |z| <= sqrt(48 ln 2) < 5.77
// log and sincospi are the accurate library functions, the products and the root separately rounded.
#pragma once
#include "common.h"

struct FdNoiseAddr {
    unsigned k0, k1;            // key
    unsigned sample_offset;     // global index of the launch's first sample (counter word 1 wraps at 2^32)
    unsigned draw, stream;
    int per;                    // elements per sample
};

// the noise address of a launch over `total` elements; the checks every noise entry point (step.hip, window.hip) shares
static inline int fd_noise_addr(const char* who, uint64_t seed, int64_t sample_offset, int per, int draw,
                                int noise_stream, unsigned long long total, FdNoiseAddr* out) {
    FD_CHECK_ARG(per > 0 && total % (unsigned long long)per == 0, FD_EINVAL,
                 "%s: sizes: per must be positive and divide the element count", who);
    FD_CHECK_ARG(sample_offset >= 0 && draw >= 0 && noise_stream >= 0, FD_EINVAL,
                 "%s: sizes: negative sample_offset, draw or stream", who);
    FD_CHECK_ARG((unsigned long long)sample_offset + total / (unsigned long long)per <= (1ull << 32), FD_EINVAL,
                 "%s: sizes: sample index past 2^32", who);
    *out = {(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned)sample_offset, (unsigned)draw,
            (unsigned)noise_stream, per};
    return FD_OK;
}

__device__ __forceinline__ void fd_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                 unsigned k1, unsigned (&w)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// two words -> the even and the odd normal of their pair
__device__ __forceinline__ void fd_normal_pair(unsigned wa, unsigned wb, float& z_even, float& z_odd) {
    const float u = __fmul_rn((float)((wa >> 8) + 1u), 0x1p-24f);
    const float f = __fmul_rn((float)(wb >> 8), 0x1p-23f);
    const float r = __fsqrt_rn(__fmul_rn(-2.f, logf(u)));
    float s, c;
    sincospif(f, &s, &c);
    z_even = __fmul_rn(r, c);
    z_odd = __fmul_rn(r, s);
}

// the words of the group that holds flat element e of the launch (sample = sample_offset + e / per)
__device__ __forceinline__ void fd_noise_words(const FdNoiseAddr& n, size_t e, unsigned (&w)[4]) {
    const unsigned idx = (unsigned)(e % (size_t)n.per);
    fd_philox4x32_10(idx >> 2, n.sample_offset + (unsigned)(e / (size_t)n.per), n.draw, n.stream, n.k0, n.k1, w);
}

// z of the V consecutive elements from flat element e on.  V = 4: e % per % 4 == 0 (per % 4 == 0 and e % 4 == 0), one
// Philox call; V = 1: the group's words, the element's pair, its lane.
template <int V>
__device__ __forceinline__ void fd_noise_normals(const FdNoiseAddr& n, size_t e, float (&z)[V]) {
    unsigned w[4];
    fd_noise_words(n, e, w);
    if constexpr (V == 4) {
        fd_normal_pair(w[0], w[1], z[0], z[1]);
        fd_normal_pair(w[2], w[3], z[2], z[3]);
    } else {
        const unsigned lane = (unsigned)(e % (size_t)n.per) & 3u;
        float ze, zo;
        fd_normal_pair(lane & 2u ? w[2] : w[0], lane & 2u ? w[3] : w[1], ze, zo);
        z[0] = lane & 1u ? zo : ze;
    }
}
