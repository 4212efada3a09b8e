// kh_stage.hpp — LDS staging of byte runs of any alignment, shared by the kernels that read or
// write unaligned byte streams (kh_find.hip: packed keys, answers, records; kh_text.hip: text,
// answers, keys): a block's input reaches LDS through aligned 16-B loads, and an output tile built
// in LDS leaves as 16-B or 4-B stores of consecutive addresses.
#pragma once
#include <hip/hip_runtime.h>

#include "kh_device.hpp"

namespace kh {

// bytes [0, bytes) at src (any alignment) -> tile[a + x], a = src & 15 (returned): aligned 16-B loads.
// The first and last load may reach up to 15 bytes outside the range, inside 16-B granules that hold
// bytes of it (as load_record_regs does). tile: 16-B aligned, >= bytes + 32. Whole block; the caller
// puts a barrier before the tile is read.
__device__ __forceinline__ uint32_t stage_bytes(const uint8_t* __restrict__ src, uint32_t bytes, uint8_t* tile) {
    const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
    const uint4* v = reinterpret_cast<const uint4*>(src - a);
    const uint32_t nvec = (a + bytes + 15u) >> 4;
    for (uint32_t i = threadIdx.x; i < nvec; i += BLOCK) reinterpret_cast<uint4*>(tile)[i] = v[i];
    return a;
}

// tile[a + x] (a = dst & 15) -> dst[x], x in [0, bytes): 16-B stores between a byte-wise head and
// tail (dst of any alignment; nothing outside the range is written). Whole block, after a barrier.
__device__ __forceinline__ void flush_bytes(uint8_t* dst, uint32_t bytes, const uint8_t* tile, uint32_t a) {
    uint32_t head = (16u - a) & 15u;
    if (head > bytes) head = bytes;
    if (threadIdx.x < head) dst[threadIdx.x] = tile[a + threadIdx.x];
    const uint32_t nvec = (bytes - head) >> 4;
    uint4* d = reinterpret_cast<uint4*>(dst + head);
    const uint4* s = reinterpret_cast<const uint4*>(tile + a + head);
    for (uint32_t i = threadIdx.x; i < nvec; i += BLOCK) d[i] = s[i];
    const uint32_t done = head + (nvec << 4);
    if (threadIdx.x < bytes - done) dst[done + threadIdx.x] = tile[a + done + threadIdx.x];
}

// L bytes of LDS at s (any alignment) -> dst (any alignment): 4-B stores of consecutive addresses
// between a byte-wise head and tail. Whole block.
__device__ __forceinline__ void copy_run(uint8_t* dst, const uint8_t* s, uint32_t L) {
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > L) head = L;
    if (threadIdx.x < head) dst[threadIdx.x] = s[threadIdx.x];
    const uint32_t nd = (L - head) >> 2;
    uint32_t* d = reinterpret_cast<uint32_t*>(dst + head);
    for (uint32_t i = threadIdx.x; i < nd; i += BLOCK) {
        const uint8_t* b = s + head + 4u * i;
        d[i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    const uint32_t done = head + 4u * nd;
    if (threadIdx.x < L - done) dst[done + threadIdx.x] = s[done + threadIdx.x];
}

}  // namespace kh
