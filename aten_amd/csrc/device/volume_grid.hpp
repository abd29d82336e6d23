// Grid media in the volume renderer: the GRID flavours of k_vol_shade and k_vol_transmit (device/volume.hpp), launched for a frame
// only when a medium material names a grid of atn_volume_set_grids.  The shade kernel delta-tracks where the homogeneous free flight
// is sampled (HeterogeneousMedium::Sample, medium.cpp:58-151), so the draws keep the reference's order; the connection walk
// ratio-tracks each segment that lies in a grid medium (EvaluateTransmittance, medium.cpp:153-202) from the connection's own sample
// stream.  The loops themselves are device/volume_grid_track.h, shared with the CPU twin.  docs/VOLUME.md, "Grid media".
#pragma once
#include "volume.hpp"

namespace atn {

#ifdef ATN_VOLUME_TU
template <int MS>
__global__ void __launch_bounds__(256) k_vol_shade_grid(PathBuffers pb, DevScene sc, FrameParams fp, atn_camera_param cam, VolArgs va, VolGridArgs vg, int32_t it)
{
#define ATN_VOL_SHADE_GRID 1
#include "volume_shade_body.hpp"
#undef ATN_VOL_SHADE_GRID
}

template <bool REFILL, bool LDSN>
__global__ void ATN_TRACE_ATTR __launch_bounds__(kTraceBlock > 256 ? kTraceBlock : 256) k_vol_transmit_grid(PathBuffers pb, DevScene sc, VolArgs va, VolGridArgs vg, int32_t it)
{
    const uint32_t count = va.counters[kVolCntConn + it];
    const VolWalkJobT<true> job{ { vg }, pb, sc, va, kEps };
    TravCounters tc{};
    trace_dispatch<false, REFILL, VolWalkJobT<true>, LDSN>(sc, count, &va.counters[kVolCntFetchT + it], job, &tc);
}
#endif  // ATN_VOLUME_TU

} // namespace atn
