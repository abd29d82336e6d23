// Node-wide SVGF (host/mgpu.hpp, MultiGpu::svgf_render; docs/MGPU_SVGF.md): what moves a shard's pixels of the four hand-over planes
// -- contributions, normal+depth, albedo+id, primary hit positions: everything the path pass hands to the filters -- to the GPU that
// filters the frame.  A shard owns every world-th 8 x 8 tile (slot_to_pixel); its pixels of a full-frame plane are rows of 8 pixels,
// 128 contiguous bytes each.  k_svgf_pack_tiles gathers them into one slot-major buffer per shard, so that the four planes travel
// in ONE peer copy; k_svgf_unpack_tiles scatters every other shard's buffer into shard 0's planes on the filtering GPU.
//
// Both are pure data movement: one thread per slot, 16-byte vector loads and stores, no atomics, no LDS.  A wave is one tile: it reads
// (pack) or writes (unpack) eight 128-byte rows per plane and the packed side is fully coalesced (64 lanes x 16 B = 1 KiB per plane).
#pragma once
#include "kernels.hpp"

namespace atn {

constexpr int kSvgfGatherPlanes = 4;        // contribs, g_nd, g_am, primary -- in this order in a packed buffer

// the tile geometry slot_to_pixel needs, for shard `rank` of `world`
ATN_DEV FrameParams svgf_gather_params(int32_t width, int32_t height, int32_t rank, int32_t world)
{
    FrameParams fp{};
    fp.width = width; fp.height = height;
    fp.tiles_x = (width + 7) / 8; fp.tiles_y = (height + 7) / 8; fp.tiles_x_rcp = udiv_rcp((uint32_t)fp.tiles_x);
    fp.rank = rank; fp.world = world;
    return fp;
}

// On shard `rank` > 0: packed[plane * n_slots + slot] = plane[pixel of slot].  A slot outside the frame (the ragged edge of an edge
// tile, a tile past the last one) reads nothing and leaves its packed entries as they are: the unpack skips the same slots.
__global__ void __launch_bounds__(256) k_svgf_pack_tiles(const float4* __restrict__ contribs, const float4* __restrict__ g_nd,
                                                         const float4* __restrict__ g_am, const float4* __restrict__ primary,
                                                         float4* __restrict__ packed, int32_t width, int32_t height,
                                                         int32_t rank, int32_t world, uint32_t n_slots)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const FrameParams fp = svgf_gather_params(width, height, rank, world);
    int32_t x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const size_t idx = (size_t)y * (size_t)width + (size_t)x;
    const float4 c = contribs[idx], nd = g_nd[idx], am = g_am[idx], pr = primary[idx];
    packed[slot] = c;
    packed[(size_t)n_slots + slot] = nd;
    packed[(size_t)2 * n_slots + slot] = am;
    packed[(size_t)3 * n_slots + slot] = pr;
}

// On the filtering GPU: gathered[(rank * 4 + plane) * n_slots + slot] -> plane[pixel of (rank, slot)] for ranks 1 .. world - 1, all
// four planes, one launch.  Rank 0 is not in the thread grid at all -- its pixels were written in place by its own path pass, so no
// pixel has two writers -- and gather memory of a slot outside the frame is never read (nobody wrote it).
__global__ void __launch_bounds__(256) k_svgf_unpack_tiles(const float4* __restrict__ gathered, float4* __restrict__ contribs,
                                                           float4* __restrict__ g_nd, float4* __restrict__ g_am, float4* __restrict__ primary,
                                                           int32_t width, int32_t height, int32_t world, uint32_t n_slots)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (uint64_t)(world - 1) * n_slots) return;
    const int32_t rank = 1 + (int32_t)(g / n_slots);        // (n_slots is a multiple of 64: a wave stays inside one rank and one tile)
    const uint32_t slot = (uint32_t)(g % n_slots);
    const FrameParams fp = svgf_gather_params(width, height, rank, world);
    int32_t x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const size_t idx = (size_t)y * (size_t)width + (size_t)x;
    const float4* src = gathered + (size_t)rank * kSvgfGatherPlanes * n_slots + slot;
    const float4 c = src[0], nd = src[(size_t)n_slots], am = src[(size_t)2 * n_slots], pr = src[(size_t)3 * n_slots];
    contribs[idx] = c;
    g_nd[idx] = nd;
    g_am[idx] = am;
    primary[idx] = pr;
}

} // namespace atn
