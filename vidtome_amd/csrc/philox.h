// Frame-keyed Gaussian noise: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3",
// SC'11; the Random123 library's philox4x32 with 10 rounds) and the Box-Muller transform on its output.  The noise of element
// e of frame `frame` at step `step` is a pure function of (seed, tag, step, frame, e): no state, no stream position, so a step
// draws it where it is used and its bits depend neither on the chunking nor on the rank or stream that runs the chunk.  The
// keying and the transform are part of the C ABI (include/vidtome_hip.h, "Frame-keyed noise"); what is restated here is the
// arithmetic.
//
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (e >> 2, frame, step, tag)          element e takes normal number e & 3 of its quad
//   round   : c = [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)], then k0 += W0, k1 += W1; ten rounds
//   normals : for (a, b) = (o0, o1) and (o2, o3):  u1 = ((a >> 9) + 0.5) 2^-23 (exact in fp32, inside (0, 1)),
//             u2 = (b >> 8) 2^-24;  r = sqrtf(-2 logf(u1));  z = r cospif(2 u2), r sinpif(2 u2)
// u1 >= 2^-24, so |z| <= sqrt(48 ln 2) = 5.7682 by construction.  The precise math functions only (the library is built
// without fast-math), and nothing here can contract into an fma.  A user of z in a 16-bit model rounds the fp32 z ONCE to the
// model dtype before anything else (normal_chunk), which is what a stored noise tensor holds.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTM_HD __host__ __device__
#else
#define VTM_HD
#endif

namespace vtm {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // the multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // the Weyl constants of the key schedule

// o = Philox4x32-10(counter c, key (k0, k1)); o may be c
VTM_HD inline void philox4x32_10(const uint32_t *c, uint32_t k0, uint32_t k1, uint32_t *o) {
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    o[0] = c0, o[1] = c1, o[2] = c2, o[3] = c3;
}

// what names a launch's noise: the key and the two counter words every element of the launch shares
struct NoiseKey {
    uint32_t k0, k1, step, tag;
};
VTM_HD inline NoiseKey noise_key(uint64_t seed, uint32_t step, uint32_t tag) {
    return NoiseKey{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), step, tag};
}

#if defined(__HIPCC__)
// the two normals of the output pair (a, b)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float &za, float &zb) {
    const float u1 = ((float)(a >> 9) + 0.5f) * 0x1p-23f;
    const float u2 = (float)(b >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    za = r * cospif(2.0f * u2);
    zb = r * sinpif(2.0f * u2);
}

// the four fp32 normals of quad `quad` (elements 4 quad .. 4 quad + 3) of frame `frame`
__device__ __forceinline__ void normal_quad(const NoiseKey &key, uint32_t quad, uint32_t frame, float *z) {
    uint32_t o[4], k0 = key.k0, k1 = key.k1, step = key.step, tag = key.tag;
    // The key and two counter words are uniform, so left alone the compiler keeps all twenty round keys (and the first round's
    // uniform products) in SGPRs across the grid-stride loop of a step kernel, which has none to spare (they spill).  Held in
    // VGPRs, the key schedule is one VALU add per round instead.
    asm volatile("" : "+v"(k0), "+v"(k1), "+v"(step), "+v"(tag));
    const uint32_t c[4] = {quad, frame, step, tag};
    philox4x32_10(c, k0, k1, o);
    box_muller(o[0], o[1], z[0], z[1]);
    box_muller(o[2], o[3], z[2], z[3]);
    // The fp32 normal is a value of its own.  Where it is converted to fp16 next, the compiler otherwise folds the last product
    // into the conversion (v_fma_mixlo_f16: the EXACT product rounded once to fp16), which is not the fp32 normal rounded to
    // fp16 when that lies on a tie -- about one element in 3000 would depend on which kernel drew it.
#pragma unroll
    for (int k = 0; k < 4; ++k) asm("" : "+v"(z[k]));
}
#endif

}  // namespace vtm
