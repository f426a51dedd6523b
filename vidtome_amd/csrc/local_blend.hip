// vtm_local_blend: the tail of a Prompt-to-Prompt LocalBlend (vidtome_amd/blend.py) on the accumulated per-word maps
// acc (G, F, h, w) fp32 and the latents x / x_src (F, C, H, W).  Per frame f and latent pixel (y, x)
//     pooled_g = max over the (2 p + 1)^2 window of acc[g, f] around (y h / H, x w / W), clipped at the border
//     mask     = OR_g ( pooled_g > threshold * max(acc[g, f]) )
//     out[f, c, y, x] = mask ? x[f, c, y, x] : x_src[f, c, y, x]
// P2P writes max_pool2d -> nearest interpolate -> divide by the maximum -> gt(threshold) -> x_src + mask * (x - x_src).  Two
// deliberate differences: the comparison is `pooled > t * max` (one fp32 multiply) instead of `pooled / max > t` -- no
// division, and an all-zero map gives an empty mask where P2P compares 0 / 0 = NaN, which is false as well; and the blend is
// a SELECT of whole elements, where `x_src + mask * (x - x_src)` rounds twice in a 16-bit model dtype.  Max-pooling commutes
// with the nearest upsampling (pool on the small grid, then look the cell up), which is what this kernel does.
// It runs once per denoising step on a few thousand latent pixels: nothing here is tuned.
//   * workgroup = 256 threads = 256 consecutive pixels of one frame; first the G maxima of the frame's maps, every thread a
//     strided share and a tree over LDS (a maximum does not depend on the order: deterministic), then the thread's pixel
//     mask, then C copies of one element each -- consecutive threads, consecutive addresses;
//   * one launch, no atomics, no workspace; every element is read and written by the same thread, so out may be x.
#include "common.h"

#include <cmath>

namespace {

constexpr int LB_NT = 256;
constexpr int LB_MAX_GROUPS = 8;

template <typename E>   // E: an unsigned integer of the element's size -- the latents are only moved
__global__ __launch_bounds__(LB_NT) void local_blend_kernel(const float *__restrict__ acc, int G, int64_t F, int h, int w,
                                                            const E *x, const E *__restrict__ x_src, E *out, int64_t C,
                                                            int H, int W, int pool, float threshold,
                                                            uint8_t *__restrict__ mask, int64_t ntiles) {
    __shared__ float sMax[LB_MAX_GROUPS][LB_NT];
    const int tid = threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x / ntiles;
    const int64_t pix = ((int64_t)blockIdx.x % ntiles) * LB_NT + tid;
    const int hw = h * w;

    for (int g = 0; g < G; ++g) {
        const float *a = acc + ((int64_t)g * F + f) * hw;
        float m = -INFINITY;
        for (int i = tid; i < hw; i += LB_NT) m = fmaxf(m, a[i]);
        sMax[g][tid] = m;
    }
    __syncthreads();
    for (int s = LB_NT / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int g = 0; g < G; ++g) sMax[g][tid] = fmaxf(sMax[g][tid], sMax[g][tid + s]);
        __syncthreads();
    }

    if (pix >= (int64_t)H * W) return;
    const int y = (int)(pix / W), xx = (int)(pix % W);
    const int cy = y / (H / h), cx = xx / (W / w);   // = y h / H, x w / W: H % h == 0, W % w == 0
    const int y0 = cy - pool < 0 ? 0 : cy - pool, y1 = cy + pool >= h ? h - 1 : cy + pool;
    const int x0 = cx - pool < 0 ? 0 : cx - pool, x1 = cx + pool >= w ? w - 1 : cx + pool;
    bool on = false;
    for (int g = 0; g < G; ++g) {
        const float *a = acc + ((int64_t)g * F + f) * hw;
        float p = -INFINITY;
        for (int yy = y0; yy <= y1; ++yy)
            for (int xc = x0; xc <= x1; ++xc) p = fmaxf(p, a[yy * w + xc]);
        const float cut = threshold * sMax[g][0];
        on = on || p > cut;
    }
    if (mask != nullptr) mask[f * H * W + pix] = on ? 1 : 0;
    const E *src = on ? x : x_src;
    const int64_t plane = (int64_t)H * W;
    for (int64_t c = 0; c < C; ++c) {
        const int64_t at = (f * C + c) * plane + pix;
        out[at] = src[at];
    }
}

}  // namespace

VTM_EXPORT int vtm_local_blend(const float *acc, int64_t G, int64_t F, int64_t h, int64_t w, const void *x, const void *x_src,
                               void *out, int dtype, int64_t C, int64_t H, int64_t W, int pool, float threshold,
                               uint8_t *mask, vtm_stream_t stream) {
    const char *who = "vtm_local_blend";
    VTM_REQUIRE(acc && x && x_src && out, "%s: null pointer", who);
    VTM_REQUIRE(G >= 1 && G <= LB_MAX_GROUPS, "%s: G = %lld, 1 .. %d groups are taken", who, (long long)G, LB_MAX_GROUPS);
    VTM_REQUIRE(F > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0, "%s: bad sizes", who);
    VTM_REQUIRE(H % h == 0 && W % w == 0, "%s: the latent %lld x %lld is not a multiple of the map %lld x %lld", who,
                (long long)H, (long long)W, (long long)h, (long long)w);
    VTM_REQUIRE(h * w < (1ll << 31) && H * W < (1ll << 31), "%s: a map or a latent plane is too large", who);
    VTM_REQUIRE(pool >= 0 && pool <= 3, "%s: pool = %d, a radius of 0 .. 3 is taken", who, pool);
    VTM_REQUIRE(std::isfinite(threshold), "%s: threshold must be finite", who);
    if (dtype != VTM_F32 && dtype != VTM_F16 && dtype != VTM_BF16)
        return vtm::fail(VTM_EINVAL, "%s: unsupported dtype %d", who, dtype);
    const int esize = dtype == VTM_F32 ? 4 : 2;
    VTM_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_src) | reinterpret_cast<uintptr_t>(out)) &
                 (uintptr_t)(esize - 1)) == 0 && (reinterpret_cast<uintptr_t>(acc) & 3) == 0, "%s: misaligned pointer", who);
    {   // out may BE x (every element is read and written by one thread); any other overlap is not taken
        const int64_t bytes = F * C * H * W * esize;
        const char *o0 = static_cast<const char *>(out), *o1 = o0 + bytes;
        for (const void *p : {x, x_src}) {
            const char *a0 = static_cast<const char *>(p), *a1 = a0 + bytes;
            VTM_REQUIRE((p == x && a0 == o0) || a1 <= o0 || o1 <= a0, "%s: out overlaps an input (it may only BE x)", who);
        }
    }
    const int64_t ntiles = vtm::cdiv(H * W, (int64_t)LB_NT);
    VTM_REQUIRE(F * ntiles < (1ll << 31), "%s: grid too large", who);
    hipStream_t s = vtm::as_stream(stream);
    const dim3 grid((unsigned)(F * ntiles)), block(LB_NT);
    if (esize == 4)
        hipLaunchKernelGGL(local_blend_kernel<uint32_t>, grid, block, 0, s, acc, (int)G, F, (int)h, (int)w, (const uint32_t *)x,
                           (const uint32_t *)x_src, (uint32_t *)out, C, (int)H, (int)W, pool, threshold, mask, ntiles);
    else
        hipLaunchKernelGGL(local_blend_kernel<uint16_t>, grid, block, 0, s, acc, (int)G, F, (int)h, (int)w, (const uint16_t *)x,
                           (const uint16_t *)x_src, (uint16_t *)out, C, (int)H, (int)W, pool, threshold, mask, ntiles);
    return vtm::launch_status(who);
}
