// The uniform grid of the mesh broad phases: n[0] x n[1] x n[2] cubic cells of side h over a box whose lower corner is lo.
// Users: the triangle grid of oai_mesh_point_distance_grid (csrc/mesh.hip), the point grid of oai_map_attributes_grid and
// oai_point_footprint_grid (csrc/thickness_map.hip) and the face grid of oai_mesh_self_intersections (csrc/mesh_quality.hip).
// The walks take a callable visit(x, y, z) and are inlined into the kernel that passes it: no function pointers.  Whether a
// search over shells may stop is the caller's test (it depends on what the cells hold and on the caller's tie-break), not the grid's.
#pragma once
#include <hip/hip_runtime.h>

namespace oai {

struct UniformGrid {
    double lo[3];
    double h, inv_h;
    int n[3];
};

inline UniformGrid make_uniform_grid(const double lo[3], double cell_size, const int dims[3]) {
    UniformGrid g;
    for (int k = 0; k < 3; ++k) { g.lo[k] = lo[k]; g.n[k] = dims[k]; }
    g.h = cell_size;
    g.inv_h = 1.0 / cell_size;
    return g;
}

// the cell of coordinate p along axis k, clamped to the grid.  This formula decides which cell a source point of
// oai_map_attributes_grid lands in, hence the order of that entry point's fp64 sums: it is part of the results.
__device__ __forceinline__ int grid_cell(const UniformGrid& g, int k, float p) {
    double t = floor(((double)p - g.lo[k]) * g.inv_h);
    t = t >= 0.0 ? t : 0.0;                        // (NaN lands in cell 0)
    t = t <= (double)(g.n[k] - 1) ? t : (double)(g.n[k] - 1);
    return (int)t;
}

// flat index of cell (x, y, z): x fastest.  Every user keeps its cell count, plus one, below 2^31.
__device__ __forceinline__ int grid_index(const UniformGrid& g, int x, int y, int z) { return (z * g.n[1] + y) * g.n[0] + x; }

// the cells of the inclusive box [x0, x1] x [y0, y1] x [z0, z1] in lexicographic order: z, then y, then x
template <class Visit>
__device__ __forceinline__ void grid_walk_box(int x0, int y0, int z0, int x1, int y1, int z1, Visit&& visit) {
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) visit(x, y, z);
}

// the largest Chebyshev shell around cell (cx, cy, cz) that still meets the grid
__device__ __forceinline__ int grid_rmax(const UniformGrid& g, int cx, int cy, int cz) {
    return max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));
}

// the cells at Chebyshev distance exactly r from cell (cx, cy, cz), clipped to the grid, each once, in (z, y, x) order.  After the
// shells 0 .. r-1, what has not been visited lies in cells at Chebyshev distance >= r, so at least (r - 1) h from any point of the
// centre cell: the bound behind every caller's stop test.
template <class Visit>
__device__ __forceinline__ void grid_walk_shell(const UniformGrid& g, int cx, int cy, int cz, int r, Visit&& visit) {
    const int z0 = max(cz - r, 0), z1 = min(cz + r, g.n[2] - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.n[1] - 1);
    const int x0 = max(cx - r, 0), x1 = min(cx + r, g.n[0] - 1);
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {      // a face of the shell's cube: the whole row
                for (int x = x0; x <= x1; ++x) visit(x, y, z);
            } else {                                                             // otherwise only the two end cells are new
                if (cx - r >= 0) visit(cx - r, y, z);
                if (cx + r < g.n[0]) visit(cx + r, y, z);
            }
        }
}

}  // namespace oai
