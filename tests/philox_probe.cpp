// Host-side probe of csrc/philox.h for tests/test_frame_noise_host.py: the integer core and the seed -> key split as the
// library compiles them, callable without a GPU.
#include <cstdint>

#include "philox.h"

extern "C" void philox_probe(const uint32_t *ctr, int64_t n, uint64_t seed, uint32_t *out, uint32_t *key_out) {
    const vtm::NoiseKey key = vtm::noise_key(seed, 0, 0);
    key_out[0] = key.k0;
    key_out[1] = key.k1;
    for (int64_t i = 0; i < n; ++i) vtm::philox4x32_10(ctr + 4 * i, key.k0, key.k1, out + 4 * i);
}
