// The planner's path search on the occupancy lattice (nav_astar.hip: k_plan_astar), written once for the kernel and for the host export
// ngp_plan_astar_host, which the CPU tests drive; plain integers only.
//
// The reference (nav/quad_helpers.py:201-258) runs A* with unit steps and a Euclidean heuristic over the 6-connected free cells.  The heuristic is
// consistent, so its path is A shortest path; WHICH of the equally short ones it returns follows from heap order on float64 f-scores.  Here:
//   1. labels: the goal gets 0; sweep d = 1, 2, ... gives label d to every free, unlabelled cell with a 6-neighbour labelled d - 1, until the start is
//      labelled or a sweep labels nothing (no path).  A cell's label is its distance to the goal.  Within sweep d a cell only reads labels d - 1, which
//      the sweep does not write, and writes d to itself: cells may be visited in any order, or all at once.
//   2. descent: from the start, move to the FIRST neighbour in the order +x, -x, +y, -y, +z, -z whose label is one less, until the goal.
// The path has the reference's length; where the shortest path is unique it is the reference's path.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGP_PLAN_HD __host__ __device__ __forceinline__
#else
#define NGP_PLAN_HD inline
#endif

static constexpr uint32_t NGP_PLAN_MAX_CELLS = 27000u;        // 30^3: 54 KB of 16-bit labels, inside the 64 KB of LDS a workgroup gets without asking
static constexpr uint16_t NGP_PLAN_FREE = 0xFFFFu;            // free, not labelled yet
static constexpr uint16_t NGP_PLAN_WALL = 0xFFFEu;            // occupied; labels proper are < 27000
enum { NGP_PLAN_PATH_OK = 0, NGP_PLAN_START_OCCUPIED = 1, NGP_PLAN_GOAL_OCCUPIED = 2, NGP_PLAN_NO_PATH = 3, NGP_PLAN_PATH_TOO_LONG = 4 };

struct ngp_plan_dims { int32_t gx, gy, gz; };                 // occupied [gx, gy, gz], x slowest

NGP_PLAN_HD int32_t ngp_plan_cell(const ngp_plan_dims& g, int32_t x, int32_t y, int32_t z) { return (x * g.gy + y) * g.gz + z; }
NGP_PLAN_HD void ngp_plan_cell_xyz(const ngp_plan_dims& g, int32_t cell, int32_t& x, int32_t& y, int32_t& z) {
    z = cell % g.gz;
    y = (cell / g.gz) % g.gy;
    x = cell / (g.gz * g.gy);
}
NGP_PLAN_HD bool ngp_plan_inside(const ngp_plan_dims& g, int32_t x, int32_t y, int32_t z) {
    return (uint32_t)x < (uint32_t)g.gx && (uint32_t)y < (uint32_t)g.gy && (uint32_t)z < (uint32_t)g.gz;
}
// neighbour k of (x, y, z) in the order +x, -x, +y, -y, +z, -z; -1 outside the grid
NGP_PLAN_HD int32_t ngp_plan_neighbour(const ngp_plan_dims& g, int32_t x, int32_t y, int32_t z, int k) {
    const int32_t step = (k & 1) ? -1 : 1;
    const int32_t nx = x + (k >> 1 == 0 ? step : 0), ny = y + (k >> 1 == 1 ? step : 0), nz = z + (k >> 1 == 2 ? step : 0);
    return ngp_plan_inside(g, nx, ny, nz) ? ngp_plan_cell(g, nx, ny, nz) : -1;
}

// sweep d on one cell: a free, unlabelled cell with a neighbour labelled d - 1 gets d; true when it did
NGP_PLAN_HD bool ngp_plan_label_step(uint16_t* labels, const ngp_plan_dims& g, int32_t cell, uint16_t d) {
    if (labels[cell] != NGP_PLAN_FREE) return false;
    int32_t x, y, z;
    ngp_plan_cell_xyz(g, cell, x, y, z);
    for (int k = 0; k < 6; k++) {
        const int32_t n = ngp_plan_neighbour(g, x, y, z, k);
        if (n >= 0 && labels[n] == (uint16_t)(d - 1u)) { labels[cell] = d; return true; }
    }
    return false;
}

// one step of the descent from a labelled cell with label > 0: the first neighbour whose label is one less (the tie-break rule); -1 if there is none,
// which cannot happen on labels that the sweeps made
NGP_PLAN_HD int32_t ngp_plan_descend(const uint16_t* labels, const ngp_plan_dims& g, int32_t cell) {
    int32_t x, y, z;
    ngp_plan_cell_xyz(g, cell, x, y, z);
    const uint16_t want = (uint16_t)(labels[cell] - 1u);
    for (int k = 0; k < 6; k++) {
        const int32_t n = ngp_plan_neighbour(g, x, y, z, k);
        if (n >= 0 && labels[n] == want) return n;
    }
    return -1;
}

// The walk from the start, by one thread: writes the n = label[start] + 1 cells start -> goal into path [cap, 3] when they fit.  Returns the status
// and n (the cells the path has, also when it does not fit; nothing is written then).
NGP_PLAN_HD int32_t ngp_plan_walk(const uint16_t* labels, const ngp_plan_dims& g, int32_t start, int32_t goal, int32_t* path, uint32_t cap, int32_t& n_cells) {
    n_cells = (int32_t)labels[start] + 1;
    if ((uint32_t)n_cells > cap) return NGP_PLAN_PATH_TOO_LONG;
    int32_t c = start;
    for (int32_t j = 0; j < n_cells && c >= 0; j++) {
        int32_t x, y, z;
        ngp_plan_cell_xyz(g, c, x, y, z);
        path[3 * j] = x; path[3 * j + 1] = y; path[3 * j + 2] = z;
        if (c == goal) break;
        c = ngp_plan_descend(labels, g, c);
    }
    return NGP_PLAN_PATH_OK;
}
