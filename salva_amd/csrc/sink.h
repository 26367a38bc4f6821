// sink.h — deleting particles by region on the device (sink.hip): the region predicates, which write one keep flag per
// row, and the stable stream compaction that moves the host-order arrays from one scan of those flags.
#pragma once
#include "common.h"
#include "mesh.h"
#include "compound.h"
#include "../../include/salva_hip.h"

namespace salva {

// The compaction's shape: a workgroup counts / scatters SINK_ROWS rows (one per thread), a scan workgroup covers the counts of
// SINK_SCAN_SPAN workgroups, and one last workgroup scans the scan workgroups' totals in a loop.  Above SINK_ROWS * SINK_SCAN_SPAN rows
// the second level carries.
constexpr uint32_t SINK_ROWS = 256;
constexpr uint32_t SINK_SCAN_SPAN = 1024;
constexpr uint32_t SINK_MAX_SLOTS = 32;  // fluids per world (tile.h MAX_MODELS)

// the rows a predicate walks: positions, the fluid of each row, and the fluid the region applies to (SALVA_HIP_ALL_FLUIDS: all)
struct SinkSrc {
    const float4* pos;
    const uint32_t* model;
    uint32_t n, slot;
    uint32_t accumulate;  // 1: a row an earlier region of the same edit has flagged stays flagged and is not counted again
};
// a validated region as the predicates read it
struct SinkRegionDev {
    int kind;             // SALVA_HIP_REGION_*
    uint32_t invert;
    float margin;
    float a[3], b[3];     // half-space: point, normal; box: mins, maxs
    float t[3], q[4];     // shape / mesh / compound: the pose
    int shape_kind;       // SALVA_HIP_SHAPE_BALL .. _CYLINDER
    float p[3];           // as SalvaHipShape::params
};

// keep[i] = 0 for every row of the region's fluid that the region selects, 1 for every other row; deleted[s] += rows of fluid s
// selected (`deleted`: SINK_MAX_SLOTS words zeroed by the caller, or nullptr).  With src.accumulate the flags of an earlier launch
// are kept: several regions applied in order to the same positions share one flag array, each counting what it adds.
// mesh / parts: what the kind needs.
void launch_sink_predicate(const SinkSrc& src, const SinkRegionDev& r, const MeshDev* mesh, const CompoundPartDev* parts, uint32_t nparts,
                           uint8_t* keep, uint32_t* deleted, hipStream_t st);
// words of scratch launch_sink_compact needs for n rows
size_t sink_scan_words(uint32_t n);
// dst[a][k] = src[a][i] for the k-th kept row i, a < narr <= 4: row i < nflag is kept when keep[i] != 0, every row in [nflag, n) is kept.
// Independent launches over the flags (counts per workgroup, the two levels of the scan of the counts, the scatter): no workgroup
// waits for another.  dst holds `cap` rows: a kept row beyond them is not written.  The number of kept rows ends up in
// scratch[sink_scan_words(n) - 1].
void launch_sink_compact(const uint8_t* keep, uint32_t nflag, uint32_t n, uint32_t* scratch, const float4* const src[4], float4* const dst[4],
                         int narr, uint32_t cap, hipStream_t st);

}  // namespace salva
