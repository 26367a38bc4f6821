// surface.h — the iso-surface of a lattice of values as an indexed triangle mesh (surface.hip): marching tetrahedra on the
// Freudenthal split of every cell.  Every mesh vertex sits on one of the seven edges a node owns, so vertices and triangles are
// numbered by two scans over per-node counts and written without atomics; the order is the contract of include/salva_hip.h.
#pragma once
#include "common.h"
#include "../../include/salva_hip.h"

namespace salva {

constexpr uint64_t SURFACE_MAX_NODES = (1ull << 31) - 2;  // (the scans run over n + 1 entries, counted in an int)
// one word per node: bits 0-6 the edges (to node + o, bit 4 ox + 2 oy + oz - 1) that carry a vertex, bits 7-9 how many they are,
// bits 10-13 the triangles (0 .. 12) of the cell the node is the min corner of
constexpr uint32_t SURFACE_MASK_BITS = 0x7fu, SURFACE_VCOUNT_SHIFT = 7, SURFACE_TCOUNT_SHIFT = 10;

// nodes as in field.h FieldQuery: node (ix, iy, iz) at origin + (float)i * spacing and at index (ix ny + iy) nz + iz
struct SurfaceLattice {
    float origin[3];
    float spacing;
    uint32_t dims[3];
    uint32_t n;  // nodes
};
// what the classification found: vertices and triangles (exact: 64-bit sums), and whether a node value was not finite
struct SurfaceTotals {
    unsigned long long nv, nt;
    uint32_t nonfinite, pad;
};

// word[i] as above for i < n, word[n] = 0; totals->nonfinite is set to 1 if a value is not finite (zeroed by the caller)
void launch_surface_classify(const float* values, float iso, const SurfaceLattice& g, uint32_t* word, SurfaceTotals* totals, hipStream_t st);
// totals->nv, ->nt = the sums of the two counts of word[0 .. n)
size_t surface_temp_bytes(uint32_t n);  // of the three calls below, for n nodes
void launch_surface_totals(void* temp, size_t temp_bytes, const uint32_t* word, uint32_t n, SurfaceTotals* totals, hipStream_t st);
// the exclusive scans of the two counts over word[0 .. n]: voff[n] = nv and toff[n] = nt, modulo 2^32 (the caller has refused more)
void launch_surface_scans(void* temp, size_t temp_bytes, const uint32_t* word, uint32_t n, uint32_t* voff, uint32_t* toff, hipStream_t st);
// the vertices (packed xyz) by owner node, then edge bit, and the triangles (three vertex indices each) by cell, then tetrahedron, then
// the order of the header's rules.  nv / nt: the totals, as bounds of what is written.
void launch_surface_emit(const float* values, float iso, const SurfaceLattice& g, const uint32_t* word, const uint32_t* voff, const uint32_t* toff,
                         uint64_t nv, uint64_t nt, float* vertices, uint32_t* triangles, hipStream_t st);
// in place: the gradient g of each vertex -> -g / |g|, the zero vector where g is zero
void launch_surface_normals(float* gradient_to_normals, uint64_t nv, hipStream_t st);
// box6 as launch_field_bbox's ({INT32_MAX x 3, INT32_MIN x 3} before), over the finite positions of the rows whose fluid is in `mask`;
// *nfinite (zeroed by the caller): how many they are
void launch_surface_bounds(const float4* st_pos, const uint32_t* st_model, uint32_t n, uint32_t mask, int32_t* box6, unsigned long long* nfinite,
                           hipStream_t st);

}  // namespace salva
