// Per-(ray, pair) work lists of the flat-scene ray queries (traverse_flat_worklist, device_scene.h): the item encoding and the
// closest-hit key.  Host and device code: tests/test_flat_worklist_cpu.py compiles these for the host.
#pragma once
#include <cstdint>

namespace mtsamd {

// An item = one primitive pair tested against one lane's ray: pair index << 6 | owner lane (pairs < 32, lanes < 64: 11 bits).
constexpr uint32_t kWlPairShift = 6u;
__host__ __device__ inline uint32_t wl_item(uint32_t owner, uint32_t pair) { return pair << kWlPairShift | owner; }
__host__ __device__ inline uint32_t wl_item_owner(uint32_t item) { return item & 63u; }
__host__ __device__ inline uint32_t wl_item_pair(uint32_t item) { return item >> kWlPairShift; }

// The items of one lane, one per set bit of its pair mask in increasing pair order, at tbl[pos], tbl[pos + 1], ...
__host__ __device__ inline void wl_push_items(uint16_t *tbl, uint32_t pos, uint32_t pairs, uint32_t lane) {
    for (; pairs != 0u; pairs &= pairs - 1u, ++pos) tbl[pos] = (uint16_t) wl_item(lane, (uint32_t) __builtin_ctz(pairs));
}

// Closest hit as a 64-bit minimum: high word = t in an unsigned order that agrees with the float order (-0 and +0 are one value),
// low word = ~primitive.  The smallest key is the smallest t and, among equal t, the largest primitive -- what the sequential loop
// over the primitives with "t <= best" keeps (later primitives win ties), whatever order the items are reduced in.  NaN is never
// a key (it fails the acceptance test), so no key equals kWlNoKey.
constexpr uint64_t kWlNoKey = ~0ull;
__host__ __device__ inline uint32_t wl_t_order(float t) {
    const uint32_t b = t == 0.0f ? 0u : __builtin_bit_cast(uint32_t, t);
    return b ^ ((uint32_t) ((int32_t) b >> 31) | 0x80000000u);
}
__host__ __device__ inline uint64_t wl_key(float t, uint32_t prim) { return (uint64_t) wl_t_order(t) << 32 | (uint32_t) ~prim; }
__host__ __device__ inline uint32_t wl_key_prim(uint64_t key) { return ~(uint32_t) key; }

}  // namespace mtsamd
