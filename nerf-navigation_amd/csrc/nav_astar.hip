// nav_astar.hip -- the planner's A* initialisation (Planner.a_star_init, nav/quad_plot.py:64-115; astar, nav/quad_helpers.py:201-258) on the device.
//
//   k_plan_occupancy   the reference's density_fn over the side^3 lattice, MaxPool3d(kernel) and `> threshold` in ONE launch: a coarse cell's kernel^3
//                      points live in one workgroup (as many cells per workgroup as fit its 256 lanes: 2 for kernel = 5), each lane evaluates its point
//                      with k_nav_density_fwd's own device functions (ngp_nav_field.h), the maximum is reduced per wave and then through LDS.  The
//                      side^3 sigma lattice (4 MB at 100^3) is never written.  sigma per point is bit for bit ngp_nav_density_forward's and max is
//                      exact, so `occupied` equals the unfused route's bit for bit.
//   k_plan_astar       the search, one workgroup: 16-bit labels of up to 27,000 cells in LDS, level-synchronous sweeps from the goal, then one lane
//                      walks from the start by the tie-break rule of ngp_plan_path.h.  Nothing traps: the outcome is result = {status, n_cells}.
#include "ngp_nav_field.h"
#include "ngp_plan_path.h"
#include <vector>

// ---------------------------------------------------------------------------
// occupancy
// ---------------------------------------------------------------------------
struct plan_rot { float m[9]; uint32_t on; };
struct plan_lattice {
    const float* ax; const float* ay; const float* az;       // [side] lattice coordinates per axis
    uint32_t k, k3;                                          // pool size, points per coarse cell
    uint32_t G, cells;                                       // coarse cells per axis, G^3
    uint32_t cpw, passes;                                    // coarse cells per workgroup; passes of 256 points over one cell when k3 > 256 (cpw = 1 then)
    float threshold;
};

// torch's max_pool3d keeps a NaN once it has met one (`val > max || isnan(val)`), and NaN > threshold is false
__device__ __forceinline__ float plan_pool(float a, float b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

__global__ __launch_bounds__(NV_BLOCK) void k_plan_occupancy(nav_params P, plan_rot R, plan_lattice L, uint8_t* __restrict__ occupied) {
    extern __shared__ float nv_smem[];
    float* col = nv_smem + 16 + threadIdx.x;
    const uint32_t t = threadIdx.x;
    const bool packed = L.k3 <= NV_BLOCK;
    const uint32_t slot = packed ? t / L.k3 : 0u;                          // this lane's cell of the workgroup; lanes past the last cell idle
    const uint32_t lc = slot < L.cpw ? slot : L.cpw - 1u;
    const uint32_t cell = blockIdx.x * L.cpw + lc;
    const uint32_t cc = cell < L.cells ? cell : L.cells - 1u;
    const uint32_t cx = cc / (L.G * L.G), cy = (cc / L.G) % L.G, cz = cc % L.G;
    float m = -INFINITY;
    for (uint32_t pass = 0; pass < L.passes; pass++) {
        const uint32_t q = packed ? t - slot * L.k3 : pass * NV_BLOCK + t;
        const bool valid = slot < L.cpw && q < L.k3 && cell < L.cells;
        const uint32_t qc = valid ? q : 0u;                                // an idle lane evaluates a point of the grid all the same: its gathers stay inside
        const uint32_t qx = qc / (L.k * L.k), qy = (qc / L.k) % L.k, qz = qc % L.k;
        const float wx = L.ax[cx * L.k + qx], wy = L.ay[cy * L.k + qy], wz = L.az[cz * L.k + qz];
        float px = wx, py = wy, pz = wz;
        if (R.on) {                                                        // p = x @ rot as k_nav_density_vj applies it (a signed permutation: exact)
            px = (wx * R.m[0] + wy * R.m[3]) + wz * R.m[6];
            py = (wx * R.m[1] + wy * R.m[4]) + wz * R.m[7];
            pz = (wx * R.m[2] + wy * R.m[5]) + wz * R.m[8];
        }
        float x0, x1, x2;
        const bool inside = nv_normalise(P, px, py, pz, x0, x1, x2);
        float out[16];
        nv_density_forward<4>(P, inside, x0, x1, x2, col, out);
        const float s = expf(out[0]);                                      // k_nav_density_fwd's sigma
        if (valid) m = plan_pool(m, s);
    }
    // ---- per wave: one butterfly per cell the wave holds points of (cells ascend with the lane) ----
    const uint32_t lane = t & 63u, wave = t >> 6;
    const uint32_t c_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)lc, 0));
    const uint32_t c_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)lc, 63));
    __syncthreads();                                                       // every lane is done with its LDS column: the space now holds the partial maxima
    float* part = nv_smem;                                                 // [4 waves][cpw]
    if (t < L.cpw) {
        #pragma unroll
        for (uint32_t w = 0; w < NV_BLOCK / 64u; w++) part[w * L.cpw + t] = -INFINITY;
    }
    __syncthreads();
    for (uint32_t c = c_lo; c <= c_hi; c++) {
        float v = lc == c ? m : -INFINITY;
        #pragma unroll
        for (int off = 32; off; off >>= 1) v = plan_pool(v, __shfl_xor(v, off));
        if (lane == 0) part[wave * L.cpw + c] = v;
    }
    __syncthreads();
    if (t < L.cpw && blockIdx.x * L.cpw + t < L.cells) {
        float r = part[t];
        #pragma unroll
        for (uint32_t w = 1; w < NV_BLOCK / 64u; w++) r = plan_pool(r, part[w * L.cpw + t]);
        occupied[blockIdx.x * L.cpw + t] = r > L.threshold ? 1 : 0;
    }
}

static constexpr size_t PLAN_OCC_LDS = sizeof(float) * (16 + NV_H * NV_BLOCK);       // k_nav_density_fwd's columns; the partial maxima (at most 4 x 256) reuse them
static constexpr uint32_t PLAN_MAX_SIDE = 1024;                                       // side^3 and kernel^3 stay below 2^31

extern "C" int ngp_plan_occupancy(const ngp_nav_field_t* f, const void* prepared, const float* axis_x, const float* axis_y, const float* axis_z,
                                  uint32_t side, uint32_t kernel, const float* rot9_host, float threshold, uint8_t* occupied, void* stream) {
    nav_params P;
    const int rc = nav_fill("plan_occupancy", f, prepared, P);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(axis_x && axis_y && axis_z && occupied, "plan_occupancy: null pointer");
    NGP_REQUIRE(kernel >= 1, "plan_occupancy: kernel must be at least 1");
    NGP_REQUIRE(side >= kernel, "plan_occupancy: side = %u is smaller than kernel = %u (no coarse cell)", side, kernel);
    NGP_REQUIRE(side <= PLAN_MAX_SIDE, "plan_occupancy: side = %u; supported up to %u", side, PLAN_MAX_SIDE);
    plan_lattice L;
    L.ax = axis_x; L.ay = axis_y; L.az = axis_z;
    L.k = kernel; L.k3 = kernel * kernel * kernel;
    L.G = side / kernel; L.cells = L.G * L.G * L.G;                        // MaxPool3d's floor: lattice points past G * kernel are not looked at
    L.cpw = L.k3 <= NV_BLOCK ? NV_BLOCK / L.k3 : 1u;
    L.passes = L.k3 <= NV_BLOCK ? 1u : ngp_div_up(L.k3, NV_BLOCK);
    L.threshold = threshold;
    plan_rot R;
    R.on = rot9_host ? 1u : 0u;
    for (int k = 0; k < 9; k++) R.m[k] = rot9_host ? rot9_host[k] : (k % 4 == 0 ? 1.0f : 0.0f);
    {
        static std::atomic<unsigned long long> devices{0};
        const int rc_lds = ngp_allow_dynamic_lds(devices, {(const void*)k_plan_occupancy}, 160 * 1024);
        if (rc_lds == NGP_LDS_NO_DEVICE) return ngp_fail(NGP_ELAUNCH, "plan_occupancy: no current device");
        if (rc_lds != NGP_LDS_OK) return ngp_fail(NGP_ELAUNCH, "plan_occupancy: cannot raise the dynamic LDS limit");
    }
    hipLaunchKernelGGL(k_plan_occupancy, dim3(ngp_div_up(L.cells, L.cpw)), dim3(NV_BLOCK), PLAN_OCC_LDS, (hipStream_t)stream, P, R, L, occupied);
    NGP_CHECK_LAUNCH("plan_occupancy");
    return NGP_OK;
}

// ---------------------------------------------------------------------------
// path search
// ---------------------------------------------------------------------------
static constexpr uint32_t PLAN_ASTAR_BLOCK = 1024;

// Control flow depends on the three flag words alone, which are written before a barrier and read after it: sweep d uses word d % 3 (bit 0: a cell was
// labelled, bit 1: the start was) and clears word (d + 1) % 3, which nobody reads any more and nobody writes before the next barrier.
__global__ __launch_bounds__(PLAN_ASTAR_BLOCK) void k_plan_astar(const uint8_t* __restrict__ occupied, ngp_plan_dims g, int32_t start, int32_t goal,
                                                                int32_t* __restrict__ path, uint32_t cap, int32_t* __restrict__ result) {
    extern __shared__ uint16_t pl_labels[];
    const int32_t n = g.gx * g.gy * g.gz;
    uint32_t* flags = (uint32_t*)(pl_labels + ((n + 1) & ~1));
    const int32_t t = (int32_t)threadIdx.x;
    for (int32_t i = t; i < n; i += (int32_t)PLAN_ASTAR_BLOCK) pl_labels[i] = occupied[i] ? NGP_PLAN_WALL : NGP_PLAN_FREE;
    if (t < 3) flags[t] = 0u;
    __syncthreads();
    int32_t status = NGP_PLAN_PATH_OK;
    if (pl_labels[start] == NGP_PLAN_WALL) status = NGP_PLAN_START_OCCUPIED;
    else if (pl_labels[goal] == NGP_PLAN_WALL) status = NGP_PLAN_GOAL_OCCUPIED;
    __syncthreads();                                                       // everyone has read the two cells before the goal's label is written
    if (status == NGP_PLAN_PATH_OK) {
        if (t == 0) pl_labels[goal] = 0;
        __syncthreads();
        if (start != goal) {
            for (uint32_t d = 1;; d++) {
                uint32_t mine = 0u;
                for (int32_t i = t; i < n; i += (int32_t)PLAN_ASTAR_BLOCK)
                    if (ngp_plan_label_step(pl_labels, g, i, (uint16_t)d)) mine |= i == start ? 3u : 1u;
                if (mine) atomicOr(&flags[d % 3u], mine);
                if (t == 0) flags[(d + 1u) % 3u] = 0u;
                __syncthreads();
                const uint32_t seen = flags[d % 3u];
                if (seen & 2u) break;
                if (!seen) { status = NGP_PLAN_NO_PATH; break; }
            }
        }
    }
    if (t == 0) {
        int32_t n_cells = 0;
        if (status == NGP_PLAN_PATH_OK) status = ngp_plan_walk(pl_labels, g, start, goal, path, cap, n_cells);
        result[0] = status;
        result[1] = n_cells;
    }
}

static int plan_astar_args(const char* who, const uint8_t* occupied, const uint32_t* dims, const int32_t* start, const int32_t* goal, const int32_t* path,
                           uint32_t cap, const int32_t* result, ngp_plan_dims& g, int32_t& s, int32_t& e) {
    NGP_REQUIRE(occupied && dims && start && goal && path && result, "%s: null pointer", who);
    NGP_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "%s: empty grid %u x %u x %u", who, dims[0], dims[1], dims[2]);
    NGP_REQUIRE(dims[0] <= NGP_PLAN_MAX_CELLS && dims[1] <= NGP_PLAN_MAX_CELLS && dims[2] <= NGP_PLAN_MAX_CELLS &&
                (uint64_t)dims[0] * dims[1] * dims[2] <= NGP_PLAN_MAX_CELLS,
                "%s: grid %u x %u x %u; supported up to %u cells (30^3: the labels live in one workgroup's LDS)", who, dims[0], dims[1], dims[2], NGP_PLAN_MAX_CELLS);
    NGP_REQUIRE(cap >= 1, "%s: cap = 0 (no room for a path)", who);
    g.gx = (int32_t)dims[0]; g.gy = (int32_t)dims[1]; g.gz = (int32_t)dims[2];
    NGP_REQUIRE(ngp_plan_inside(g, start[0], start[1], start[2]), "%s: start (%d, %d, %d) is outside the grid", who, start[0], start[1], start[2]);
    NGP_REQUIRE(ngp_plan_inside(g, goal[0], goal[1], goal[2]), "%s: goal (%d, %d, %d) is outside the grid", who, goal[0], goal[1], goal[2]);
    s = ngp_plan_cell(g, start[0], start[1], start[2]);
    e = ngp_plan_cell(g, goal[0], goal[1], goal[2]);
    return NGP_OK;
}

extern "C" int ngp_plan_astar(const uint8_t* occupied, const uint32_t* dims_host, const int32_t* start_host, const int32_t* goal_host, int32_t* path,
                              uint32_t cap, int32_t* result, void* stream) {
    ngp_plan_dims g;
    int32_t s, e;
    const int rc = plan_astar_args("plan_astar", occupied, dims_host, start_host, goal_host, path, cap, result, g, s, e);
    if (rc != NGP_OK) return rc;
    const uint32_t n = (uint32_t)(g.gx * g.gy * g.gz);
    const size_t lds = sizeof(uint16_t) * ((n + 1u) & ~1u) + 3 * sizeof(uint32_t);
    hipLaunchKernelGGL(k_plan_astar, dim3(1), dim3(PLAN_ASTAR_BLOCK), lds, (hipStream_t)stream, occupied, g, s, e, path, cap, result);
    NGP_CHECK_LAUNCH("plan_astar");
    return NGP_OK;
}

// the same search by the same functions, cell after cell on the host (all pointers host memory)
extern "C" int ngp_plan_astar_host(const uint8_t* occupied, const uint32_t* dims_host, const int32_t* start_host, const int32_t* goal_host, int32_t* path,
                                   uint32_t cap, int32_t* result) {
    ngp_plan_dims g;
    int32_t s, e;
    const int rc = plan_astar_args("plan_astar_host", occupied, dims_host, start_host, goal_host, path, cap, result, g, s, e);
    if (rc != NGP_OK) return rc;
    const int32_t n = g.gx * g.gy * g.gz;
    std::vector<uint16_t> labels((size_t)n);
    for (int32_t i = 0; i < n; i++) labels[(size_t)i] = occupied[i] ? NGP_PLAN_WALL : NGP_PLAN_FREE;
    int32_t status = NGP_PLAN_PATH_OK, n_cells = 0;
    if (labels[(size_t)s] == NGP_PLAN_WALL) status = NGP_PLAN_START_OCCUPIED;
    else if (labels[(size_t)e] == NGP_PLAN_WALL) status = NGP_PLAN_GOAL_OCCUPIED;
    if (status == NGP_PLAN_PATH_OK) {
        labels[(size_t)e] = 0;
        for (uint32_t d = 1; labels[(size_t)s] == NGP_PLAN_FREE; d++) {
            bool grew = false;
            for (int32_t i = 0; i < n; i++) grew |= ngp_plan_label_step(labels.data(), g, i, (uint16_t)d);
            if (!grew) { status = NGP_PLAN_NO_PATH; break; }
        }
    }
    if (status == NGP_PLAN_PATH_OK) status = ngp_plan_walk(labels.data(), g, s, e, path, cap, n_cells);
    result[0] = status;
    result[1] = n_cells;
    return NGP_OK;
}
