// vtm_frame_noise: frame-keyed N(0, 1) noise as a tensor -- out[s, f, e] is the normal of element e of frame row(f) at step
// step0 + s, a pure function of (seed, tag, step, frame, e) (philox.h; the keying is the C ABI's, include/vidtome_hip.h).  It
// is what the keyed steps (vtm_guided_step_keyed, vtm_solver_step_keyed) draw in place, for the callers that want the tensor:
// the inversion's noise levels, the initial latents, a stored-noise run to compare against.
//
// One thread per QUAD, the four normals of one Philox call: the store is the quad, 16 bytes in fp32 and 8 in a 16-bit dtype,
// when a frame is whole quads (E % 4 == 0) and `out` is aligned to the store, and element by element otherwise (the last quad
// of a frame may then be partial); which of the two changes no bit.  No workspace, no atomics.
// vtm_philox_bits: the integer core alone on caller-given counters, so a test can pin it exactly on the device.
#include "common.h"
#include "step_core.h"

namespace {

constexpr int FN_THREADS = 256;

template <typename T, bool VEC>
__global__ __launch_bounds__(FN_THREADS) void frame_noise_kernel(T *__restrict__ out, int64_t S, int64_t F, int64_t E,
                                                                 const int32_t *__restrict__ frame_ids, int64_t frame0,
                                                                 vtm::NoiseKey key) {
    const int64_t quads = (E + 3) / 4, total = S * F * quads;
    const int64_t i = (int64_t)blockIdx.x * FN_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t sf = i / quads, q = i - sf * quads, s = sf / F, f = sf - s * F;
    const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
    key.step += (uint32_t)s;
    float z[4];
    vtm::normal_quad(key, (uint32_t)q, (uint32_t)(frame0 + row), z);
    T *p = out + sf * E + q * 4;
    if constexpr (VEC) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4 *>(p) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
            uint2 raw;
            T *e = reinterpret_cast<T *>(&raw);
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = vtm::from_f32<T>(z[k]);
            *reinterpret_cast<uint2 *>(p) = raw;
        }
    } else {
        const int n = (int)std::min<int64_t>(4, E - q * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = vtm::from_f32<T>(z[k]);
    }
}

__global__ __launch_bounds__(FN_THREADS) void philox_bits_kernel(const uint32_t *__restrict__ ctr, int64_t n, uint32_t k0,
                                                                 uint32_t k1, uint32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * FN_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint4 c = *reinterpret_cast<const uint4 *>(ctr + 4 * i);
    const uint32_t in[4] = {c.x, c.y, c.z, c.w};
    uint32_t o[4];
    vtm::philox4x32_10(in, k0, k1, o);
    *reinterpret_cast<uint4 *>(out + 4 * i) = make_uint4(o[0], o[1], o[2], o[3]);
}

constexpr int64_t MAX_THREADS = (int64_t(1) << 32) - FN_THREADS;      // of one launch

}  // namespace

VTM_EXPORT int vtm_frame_noise(void *out, int dtype, int64_t S, int64_t F, int64_t E, const int32_t *frame_ids, int64_t frame0,
                               uint64_t seed, uint32_t step0, uint32_t tag, vtm_stream_t stream) {
    const char *who = "vtm_frame_noise";
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(out, "%s: out is required", who);
    VTM_REQUIRE(S >= 0 && S <= (int64_t(1) << 32) && F >= 0 && F <= (1 << 20) && E >= 1,
                "%s: bad sizes S = %lld, F = %lld, E = %lld", who, (long long)S, (long long)F, (long long)E);
    if (const int rc = vtm::check_keyed(who, frame0, E)) return rc;
    if (S == 0 || F == 0) return VTM_OK;
    const int64_t quads = vtm::cdiv(E, 4);
    VTM_REQUIRE(S <= MAX_THREADS / F && S * F <= MAX_THREADS / quads, "%s: S * F * ceil(E / 4) = %lld * %lld * %lld quads exceed one launch",
                who, (long long)S, (long long)F, (long long)quads);
    const int64_t total = S * F * quads;
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        const bool vec = E % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & (4 * sizeof(T) - 1)) == 0;
        auto *kernel = vec ? frame_noise_kernel<T, true> : frame_noise_kernel<T, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)vtm::cdiv(total, FN_THREADS)), dim3(FN_THREADS), 0, vtm::as_stream(stream),
                           (T *)out, S, F, E, frame_ids, frame0, vtm::noise_key(seed, step0, tag));
        return (int)VTM_OK;
    });
    if (rc != VTM_OK) return rc;
    return vtm::launch_status(who);
}

VTM_EXPORT int vtm_philox_bits(const uint32_t *ctr, int64_t n, uint64_t seed, uint32_t *out, vtm_stream_t stream) {
    const char *who = "vtm_philox_bits";
    VTM_REQUIRE(ctr && out, "%s: ctr and out are required", who);
    VTM_REQUIRE(n >= 0 && n <= MAX_THREADS, "%s: n = %lld outside [0, 2^32 - %d]", who, (long long)n, FN_THREADS);
    VTM_REQUIRE(vtm::aligned16(ctr) && vtm::aligned16(out), "%s: ctr and out must be 16-byte aligned", who);
    if (n == 0) return VTM_OK;
    const vtm::NoiseKey key = vtm::noise_key(seed, 0, 0);
    hipLaunchKernelGGL(philox_bits_kernel, dim3((unsigned)vtm::cdiv(n, FN_THREADS)), dim3(FN_THREADS), 0, vtm::as_stream(stream),
                       ctr, n, key.k0, key.k1, out);
    return vtm::launch_status(who);
}
