// nav_frame.hip -- one frame of NeRFRenderer.run_cuda's inference branch (nerf/renderer.py:325-374) of the DEFAULT float32 field
// (nerf/network.py, the model the nav loop flies in) in ONE launch: the counterpart of render_fused.hip's k_render_frame_multi, whose
// semantics it shares word for word (include/ngp_hip.h): one resumable march per ray from `near`, at most max_steps samples,
// a ray stops after the sample whose incoming T is below 1e-4.
//
// Stage 1: everything on the vector ALU, float32 throughout, with the field of nav_field.hip (ngp_nav_field.h).
//   march / composite : lane <-> ray.  A persistent 256-thread workgroup holds 256 rays; a free lane takes the next ray of ONE global queue
//                       (8x8 pixel tiles when the rays are an image).  Per round a lane marches up to NVF_S samples of its ray into LDS
//                       slots (x, y, z, t), probing the bitfield cell by cell with ngp_march.h's ngp_point::at / cell_exit / ngp_advance:
//                       the sample positions are the per-op march's bits.
//   field evaluation  : lane <-> sample.  The round's filled slots are listed by a block scan, and the 256 lanes evaluate 256 listed
//                       samples per pass, whichever ray they belong to: 16 x 8 float2 gathers, 32-64-16, SH16 ++ geo15, 31-64-64-3,
//                       weights through the scalar cache, the activation column in LDS (nv_density_forward, nv_color_forward).
//                       (sigma * density_scale, r, g, b) overwrite the slot.
//   composite         : each ray's lane composites its samples in order (kernel_composite_rays' arithmetic, raymarching.cu:865-896);
//                       what it marched behind the sample that saturated it is discarded.
// No workgroup waits for another: the only shared state is the queue counter and the four statistics words (integer atomics).  Every
// loop is bounded by max_steps, far, the probe budget or the queue length.  No float atomics: two launches give the same bits.
#include "ngp_nav_field.h"
#include "ngp_march.h"
#include "ngp_camera.h"

// Build-time knobs, A/B-measured on an MI355X with tools/time_default_frame.py (800x800 S-ring frame of the hand-set nav model, 100 frames each, ms per frame):
//   NVF_U (levels in flight) 4: 24.9 | 2: 22.5 | 1: 17.1        NVF_PROBES at U = 4: 16: 35.6 | 32: 30.3 | 64: 24.9; at U = 1: 64: 17.1 | 128: 18.4 | 256: 20.2 | 1024: 20.0
//   NVF_S at U = 4: 2: 30.5 | 3: 24.9; one workgroup per CU with 8 slots: 31.2, with 12: 30.0 (U = 1, 8 slots, 256 probes: 28.7)
#ifndef NVF_S
#define NVF_S 3                        // samples a lane may march per round: 256 x NVF_S slots of 16 B beside the 64 KiB activation columns;
#endif                                 // 3 keeps a workgroup under 80 KiB of LDS, i.e. two workgroups (2 waves per SIMD) on a CU
#ifndef NVF_PROBES
#define NVF_PROBES 64                  // cells a lane may probe per round while it looks for its samples: fewer and the rounds run half empty (every
#endif                                 // round costs a pass over up to 256 samples however few it holds), more and the lanes that are full wait for one that is not
#ifndef NVF_WG_PER_CU
#define NVF_WG_PER_CU 2                // workgroups that share a CU (= waves per SIMD): what the LDS carve allows
#endif
#ifndef NVF_U
#define NVF_U 1                        // levels of the hash grid whose gathers may overlap (nv_hidden): one at a time, as in the run kernels.  Unrolling four
#endif                                 // levels costs 72 registers and four copies of the first layer's 128 multiply-adds per level in the instruction stream
static constexpr uint32_t NVF_BLOCK = NV_BLOCK;                          // the nv_* functions stride their LDS column by NV_BLOCK
static constexpr uint32_t NVF_SLOTS = NVF_BLOCK * NVF_S;
static constexpr uint32_t NVF_LDS_HEAD = 16;                             // floats: scan scratch
static constexpr uint32_t NVF_LDS_COL = NV_H * NVF_BLOCK;                // floats: the activation columns
static constexpr size_t NVF_LDS = sizeof(float) * (NVF_LDS_HEAD + NVF_LDS_COL) + sizeof(float4) * NVF_SLOTS + sizeof(uint32_t) * NVF_BLOCK +
                                  sizeof(uint16_t) * NVF_SLOTS;          // head | columns | slots | ray of each lane | list of filled slots
static_assert(NVF_S >= 1 && NVF_SLOTS <= 65536, "slot ids are 16 bits");
static_assert(NVF_LDS <= 160 * 1024, "LDS carve exceeds 160 KiB");

struct nvf_frame {
    const float* rays_o; const float* rays_d; uint32_t N;               // rays_o == null: the rays are those of `cam` (pixel = ray id)
    ngp_camera cam;
    float aabb[6]; float min_near;
    const uint8_t* bitfield; uint32_t C, H;
    float dt_gamma; uint32_t max_steps;
    float bg[3];
    float* image; float* depth; float* weights_sum;
    uint32_t* stats; uint32_t* queue;
    uint32_t tile_w;                                                     // image width in pixels when the rays are a row-major image (8x8 tile order), else 0
};

// the view ngp_march.h's templates read: the ray (per lane) and the march constants (uniform), same formulas as ngp_march_t::setup.
// The launcher requires a power-of-two grid, so the scalings by H take their one-multiply forms (hHf = 0.5 H, r2H = 2 / H: powers of two).
struct nvf_view {
    static constexpr bool pow2_grid = true;
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
    float bound, rbound, dt_gamma, dt_min, dt_max, H3, hHf, r2H, Hm1;
    int Cm1;
    __device__ __forceinline__ int mip(int e) const { return min(max(e, 0), Cm1); }
};

__device__ __forceinline__ float nvf_uniform(float v) {                  // a wave-uniform value computed by the vector ALU -> SGPR
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// ray id -> origin and direction: explicit rays, or the camera (get_rays fused, nerf/utils.py:98-108)
__device__ __forceinline__ void nvf_ray_od(const nvf_frame& F, uint32_t ray, float o[3], float d[3]) {
    if (F.rays_o) {
        #pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = F.rays_o[3ull * ray + k]; d[k] = F.rays_d[3ull * ray + k]; }
    } else {
        o[0] = F.cam.t[0]; o[1] = F.cam.t[1]; o[2] = F.cam.t[2];
        ngp_camera_ray(F.cam, ray, d);
    }
}

// queue index -> ray id: with tile_w set consecutive indices walk 8x8 pixel tiles, 16 consecutive ones a 4x4 patch (neighbouring rays
// gather neighbouring cells); otherwise the identity
__device__ __forceinline__ uint32_t nvf_ray_of(uint32_t idx, uint32_t tile_w) {
    if (tile_w == 0) return idx;
    const uint32_t tile = idx >> 6, in = idx & 63u, tiles_x = tile_w >> 3;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t p = in >> 4, s = in & 15u;
    const uint32_t px = (p & 1u) * 4 + (s & 3u), py = (p >> 1) * 4 + (s >> 2);
    return (ty * 8 + py) * tile_w + tx * 8 + px;
}

__global__ __launch_bounds__(NVF_BLOCK, NVF_WG_PER_CU) void k_nav_render_frame(nav_params P, nvf_frame F) {
    extern __shared__ __attribute__((aligned(16))) float nvf_smem[];
    uint32_t* lds4 = reinterpret_cast<uint32_t*>(nvf_smem);
    float* col = nvf_smem + NVF_LDS_HEAD + threadIdx.x;                  // this lane's column of the [64][256] scratch
    float4* smp = reinterpret_cast<float4*>(nvf_smem + NVF_LDS_HEAD + NVF_LDS_COL);
    uint32_t* lds_ray = reinterpret_cast<uint32_t*>(smp + NVF_SLOTS);
    uint16_t* list = reinterpret_cast<uint16_t*>(lds_ray + NVF_BLOCK);
    float4* my_smp = smp + threadIdx.x * NVF_S;
    const uint32_t lane = threadIdx.x & 63u;

    nvf_view V;
    V.bound = P.bound; V.rbound = nvf_uniform(1.0f / P.bound); V.dt_gamma = F.dt_gamma;
    const float Hf = nvf_uniform((float)F.H);
    V.hHf = nvf_uniform(0.5f * Hf); V.Cm1 = (int)F.C - 1; V.Hm1 = nvf_uniform((float)(F.H - 1));
    V.r2H = nvf_uniform(2.0f * (1.0f / Hf));
    V.H3 = nvf_uniform((float)(F.H * F.H * F.H));
    V.dt_min = nvf_uniform((2.0f * 1.7320508075688772f) / (float)F.max_steps);
    V.dt_max = nvf_uniform(((2.0f * 1.7320508075688772f) * (float)(1 << (F.C - 1))) / Hf);
    V.ox = V.oy = V.oz = 0.0f; V.dx = V.dy = V.dz = 1.0f; V.rdx = V.rdy = V.rdz = 1.0f;
    const uint32_t last_bit = F.C * F.H * F.H * F.H - 1u;                // the bitfield's last cell (host: C * H^3 <= 2^30)

    bool active = false, exhausted = false;
    uint32_t ray = 0, nsamp = 0;
    float t = 0, last_t = 0, near = 0, far = 0;
    float ws = 0, dacc = 0, cr = 0, cg = 0, cb = 0, tcomp = 0;
    uint32_t n_samples = 0, n_capped = 0, n_hit = 0, n_eval = 0;
    volatile uint32_t* vote = lds4 + 8;                                  // three words of the head, behind the scan's four
    uint32_t round = 0;
    if (threadIdx.x < 3) vote[threadIdx.x] = 0u;
    __syncthreads();

    for (;;) {
        // ---- refill: every free lane takes the next ray of the queue ----
        if (!exhausted) {
            const unsigned long long need = __ballot(!active);
            if (need) {
                const uint32_t cnt = (uint32_t)__popcll(need);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(F.queue, cnt);
                base = __shfl(base, 0, 64);
                if (!active) {
                    const uint32_t idx = base + (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
                    if (idx < F.N) {
                        ray = nvf_ray_of(idx, F.tile_w);
                        float o[3], d[3];
                        nvf_ray_od(F, ray, o, d);
                        ngp_near_far_inline(o, d, F.aabb, F.min_near, near, far);
                        V.ox = o[0]; V.oy = o[1]; V.oz = o[2];
                        V.dx = d[0]; V.dy = d[1]; V.dz = d[2];
                        V.rdx = 1.0f / V.dx; V.rdy = 1.0f / V.dy; V.rdz = 1.0f / V.dz;
                        t = near; last_t = near; tcomp = near;
                        ws = 0; dacc = 0; cr = 0; cg = 0; cb = 0; nsamp = 0;
                        lds_ray[threadIdx.x] = ray;
                        active = true;
                    }
                }
                if (base + cnt >= F.N) exhausted = true;                 // the queue has run dry under this wave (uniform: base and cnt are)
            }
        }
        // the workgroup's vote: bit 0 = some lane holds a ray, bit 1 = some wave may still draw.  Three words in turn: the word of round i + 1 is
        // cleared before this round's barrier, when every lane has read it for the last time (in round i - 2, before the barrier of round i - 1)
        // and none adds to it yet.  (The library's __syncthreads_or would do, but brings 256 bytes of static LDS.)
        {
            const uint32_t mine = (__ballot(active) ? 1u : 0u) | (exhausted ? 0u : 2u);
            if (threadIdx.x == 0) vote[(round + 1u) % 3u] = 0u;
            if (lane == 0 && mine) atomicOr(const_cast<uint32_t*>(&vote[round % 3u]), mine);
            __syncthreads();                                             // (also: lds_ray is visible to the evaluating lanes)
            const uint32_t all = vote[round % 3u];
            round++;
            if (!(all & 1u)) {
                if (!(all & 2u)) break;
                continue;                                                // a wave that may still draw does so, and gets rays or runs dry
            }
        }

        // ---- march: up to NVF_S samples of this lane's ray, within the probe budget ----
        uint32_t cnt = 0;
        bool ended = false;
        if (active) {
            uint32_t probes = 0;
            for (;;) {
                if (!(t < far && nsamp < F.max_steps)) { ended = true; break; }
                const float t_before = t;
                ngp_point<nvf_view> r;
                r.at(V, t);
                const uint32_t mort = ngp_morton3((uint32_t)r.nx, (uint32_t)r.ny, (uint32_t)r.nz);
                // the reference's cell index, formed in binary32 (raymarching.cu:783-784); where that rounds beyond the last cell it reads the last one
                uint32_t index = (uint32_t)((float)r.level * V.H3 + (float)mort);
                index = index < last_bit ? index : last_bit;
                if ((F.bitfield[index >> 3] >> (index & 7u)) & 1u) {
                    my_smp[cnt] = make_float4(r.x, r.y, r.z, t);
                    t += r.dt;
                    nsamp++;
                    if (++cnt >= NVF_S) break;
                } else {
                    float tp;
                    t = ngp_advance(V, t, r.cell_exit(V, t), tp);
                }
                // a ray parameter so large that a step no longer changes it (an origin millions of box widths away) would keep the reference's
                // march, and this loop, at the same point for ever: such a ray ends here
                if (!(t > t_before)) { ended = true; break; }
                if (++probes >= NVF_PROBES) break;
            }
        }
        float ts[NVF_S];                                                 // the samples' ray parameters: the slots are about to be overwritten
        #pragma unroll
        for (int k = 0; k < NVF_S; k++) ts[k] = (uint32_t)k < cnt ? my_smp[k].w : 0.0f;

        // ---- list the filled slots (block scan of the counts) ----
        uint32_t total;
        const uint32_t first = ngp_block_inclusive_scan<NVF_BLOCK / 64>(cnt, lds4, total) - cnt;
        #pragma unroll
        for (int k = 0; k < NVF_S; k++)
            if ((uint32_t)k < cnt) list[first + k] = (uint16_t)(threadIdx.x * NVF_S + k);
        __syncthreads();

        // ---- field evaluation: lane <-> listed sample ----
        for (uint32_t p0 = 0; p0 < total; p0 += NVF_BLOCK) {
            const uint32_t i = p0 + threadIdx.x;
            const bool live = i < total;
            const uint32_t slot = list[live ? i : 0u];
            const float4 q = smp[slot];
            float o[3], d[3];
            nvf_ray_od(F, lds_ray[slot / NVF_S], o, d);
            float x0, x1, x2;
            const bool inside = nv_normalise(P, q.x, q.y, q.z, x0, x1, x2);
            float out[16];
            nv_density_forward<NVF_U>(P, inside, x0, x1, x2, col, out);
            const float sigma = expf(out[0]) * P.density_scale;          // trunc_exp forward (activation.py:9-10), times the renderer's density_scale (renderer.py:361)
            float geo[NV_GEO], rgb[3];
            #pragma unroll
            for (int m = 0; m < NV_GEO; m++) geo[m] = out[1 + m];
            uint64_t ma, mb;
            nv_color_forward(P, d[0], d[1], d[2], geo, col, rgb, ma, mb);
            if (live) { smp[slot] = make_float4(sigma, rgb[0], rgb[1], rgb[2]); n_eval++; }
        }
        __syncthreads();

        // ---- composite this lane's samples in order (kernel_composite_rays, raymarching.cu:865-896) ----
        bool done = false;
        #pragma unroll
        for (int k = 0; k < NVF_S; k++) {
            if ((uint32_t)k < cnt && !done) {
                const float4 r = my_smp[k];
                const float dt = ngp_clampf(ts[k] * V.dt_gamma, V.dt_min, V.dt_max);
                const float ta = ts[k] + dt;
                const float d1 = ta - last_t;
                last_t = ta;
                n_samples++;
                const float alpha = 1.0f - ngp_expf(-r.x * dt);
                const float T = 1 - ws;
                const float w = alpha * T;
                ws += w;
                tcomp += d1;
                dacc += w * tcomp;
                cr += w * r.y; cg += w * r.z; cb += w * r.w;
                if ((double)T < 1e-4) done = true;                       // samples marched beyond this one are discarded
            }
        }
        if (active) {
            const bool capped = !done && ended && nsamp >= F.max_steps && t < far;
            if (ended) done = true;
            if (done) {
                F.image[3ull * ray] = cr + (1 - ws) * F.bg[0];
                F.image[3ull * ray + 1] = cg + (1 - ws) * F.bg[1];
                F.image[3ull * ray + 2] = cb + (1 - ws) * F.bg[2];
                F.depth[ray] = fmaxf(dacc - near, 0.0f) / (far - near);
                F.weights_sum[ray] = ws;
                n_capped += capped ? 1u : 0u;
                n_hit += nsamp > 0 ? 1u : 0u;
                active = false;
            }
        }
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_samples += __shfl_down(n_samples, off, 64);
        n_capped += __shfl_down(n_capped, off, 64);
        n_hit += __shfl_down(n_hit, off, 64);
        n_eval += __shfl_down(n_eval, off, 64);
    }
    if (lane == 0 && n_samples) atomicAdd(F.stats, n_samples);
    if (lane == 0 && n_capped) atomicAdd(F.stats + 1, n_capped);
    if (lane == 0 && n_hit) atomicAdd(F.stats + 2, n_hit);
    if (lane == 0 && n_eval) atomicAdd(F.stats + 3, n_eval);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Frame workspace: a header of 64 words, word 0 = the ray queue's head (zeroed by the call); the same for every N.
static constexpr size_t NVF_WS_HEADER_WORDS = 64;
struct nvf_ws { uint32_t* header; size_t total; };
static nvf_ws nvf_layout(uint32_t N, void* base) {
    (void)N;
    ngp_carver c(base);
    return {c.take<uint32_t>(NVF_WS_HEADER_WORDS, 1), c.total()};
}
extern "C" size_t ngp_nav_render_frame_workspace(uint32_t N) { return nvf_layout(N, nullptr).total; }

static int nvf_fill_camera(const float* pose_host, const float* intrinsics_host, uint32_t H, uint32_t W, ngp_camera& cam) {
    NGP_REQUIRE(pose_host && intrinsics_host, "nav_render_frame_camera: pose / intrinsics are host pointers and must not be null");
    NGP_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= 0xFFFFFFFFull, "nav_render_frame_camera: bad image size");
    NGP_REQUIRE(intrinsics_host[0] != 0.0f && intrinsics_host[1] != 0.0f, "nav_render_frame_camera: zero focal length");
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.r[3 * r + c] = pose_host[4 * r + c];
        cam.t[r] = pose_host[4 * r + 3];
    }
    cam.fx = intrinsics_host[0]; cam.fy = intrinsics_host[1]; cam.cx = intrinsics_host[2]; cam.cy = intrinsics_host[3];
    cam.W = W; cam.H = H;
    return NGP_OK;
}

static int nvf_render_frame(const char* who, const ngp_nav_field_t* field_host, const void* prepared, const float* rays_o, const float* rays_d,
                            const ngp_camera* cam, uint32_t N, uint32_t image_width, const float* aabb_host, float min_near, const uint8_t* bitfield,
                            uint32_t C, uint32_t Hgrid, float dt_gamma, uint32_t max_steps, const float* bg_color3_host,
                            float* image, float* depth, float* weights_sum, uint32_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
    // every refusal comes before anything reaches the device
    nav_params P;
    int rc = nav_fill(who, field_host, prepared, P);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE((cam || (rays_o && rays_d)) && aabb_host && bg_color3_host && bitfield && image && depth && weights_sum && stats && workspace,
                "%s: null pointer", who);
    NGP_REQUIRE(C >= 1 && C <= 16 && Hgrid >= 1 && Hgrid <= 1024 && max_steps >= 1, "%s: bad C/H/max_steps", who);
    // cells are addressed by Morton index: for a grid size that is not a power of two the index of a cell can lie beyond the end of the bitfield
    NGP_REQUIRE((Hgrid & (Hgrid - 1u)) == 0u, "%s: the grid size must be a power of two (cells are addressed by Morton index)", who);
    NGP_REQUIRE((uint64_t)C * Hgrid * Hgrid * Hgrid <= (1ull << 30), "%s: the occupancy grid has more than 2^30 cells", who);
    // the bitfield is C * H^3 / 8 bytes: a grid of fewer bits than a byte holds (H = 1, C not a multiple of 8) has no whole number of them
    NGP_REQUIRE(((uint64_t)C * Hgrid * Hgrid * Hgrid) % 8u == 0u, "%s: the occupancy grid's C * H^3 bits are not a whole number of bytes", who);
    NGP_REQUIRE(N <= 0xFFF00000u, "%s: too many rays", who);            // the queue's head runs past N by at most 64 per wave
    const nvf_ws ws = nvf_layout(N, workspace);
    if (workspace_bytes < ws.total)
        return ngp_fail(NGP_EWORKSPACE, "%s: workspace of %zu bytes, needs ngp_nav_render_frame_workspace(N) = %zu", who, workspace_bytes, ws.total);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), s) != hipSuccess || hipMemsetAsync(ws.header, 0, NVF_WS_HEADER_WORDS * 4, s) != hipSuccess)
        return ngp_fail(NGP_ELAUNCH, "%s: memset failed", who);
    if (N == 0) return NGP_OK;
    nvf_frame F;
    F.rays_o = cam ? nullptr : rays_o; F.rays_d = cam ? nullptr : rays_d; F.N = N;
    F.cam = cam ? *cam : ngp_camera{};
    for (int i = 0; i < 6; i++) F.aabb[i] = aabb_host[i];
    F.min_near = min_near; F.bitfield = bitfield; F.C = C; F.H = Hgrid;
    F.dt_gamma = dt_gamma; F.max_steps = max_steps;
    for (int i = 0; i < 3; i++) F.bg[i] = bg_color3_host[i];
    F.image = image; F.depth = depth; F.weights_sum = weights_sum;
    F.stats = stats; F.queue = ws.header;
    F.tile_w = 0;
    if (image_width >= 8 && image_width % 8 == 0 && N % image_width == 0 && (N / image_width) % 8 == 0) F.tile_w = image_width;
    // the kernel uses more than the default 64 KiB of dynamic LDS; the raised limit is a per-device function attribute
    static std::atomic<unsigned long long> devices{0};
    const int rc_lds = ngp_allow_dynamic_lds(devices, {(const void*)k_nav_render_frame}, NVF_LDS);
    if (rc_lds == NGP_LDS_NO_DEVICE) return ngp_fail(NGP_ELAUNCH, "%s: no current device", who);
    if (rc_lds != NGP_LDS_OK) return ngp_fail(NGP_ELAUNCH, "%s: cannot raise the dynamic LDS limit", who);
    // persistent grid: NVF_WG_PER_CU workgroups per CU, fewer when the frame is small
    uint32_t blocks = 256 * NVF_WG_PER_CU;
    const uint32_t need = ngp_div_up(N, NVF_BLOCK);
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(k_nav_render_frame, dim3(blocks), dim3(NVF_BLOCK), NVF_LDS, s, P, F);
    NGP_CHECK_LAUNCH(who);
    return NGP_OK;
}

extern "C" int ngp_nav_render_frame(const ngp_nav_field_t* field_host, const void* prepared,
                                    const float* rays_o, const float* rays_d, uint32_t N, uint32_t image_width,
                                    const float* aabb_host, float min_near, const uint8_t* bitfield, uint32_t C, uint32_t Hgrid,
                                    float dt_gamma, uint32_t max_steps, const float* bg_color3_host,
                                    float* image, float* depth, float* weights_sum, uint32_t* stats,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return nvf_render_frame("nav_render_frame", field_host, prepared, rays_o, rays_d, nullptr, N, image_width, aabb_host, min_near, bitfield, C, Hgrid,
                            dt_gamma, max_steps, bg_color3_host, image, depth, weights_sum, stats, workspace, workspace_bytes, stream);
}

// The same frame from a camera instead of ray arrays: get_rays (nerf/utils.py:53-116, full-image branch) runs inside the kernel's refill, one
// ray per pixel in row-major order (ngp_camera.h); bit-identical to ngp_get_rays + ngp_nav_render_frame.
extern "C" int ngp_nav_render_frame_camera(const ngp_nav_field_t* field_host, const void* prepared,
                                           const float* pose_host, const float* intrinsics_host, uint32_t H, uint32_t W,
                                           const float* aabb_host, float min_near, const uint8_t* bitfield, uint32_t C, uint32_t Hgrid,
                                           float dt_gamma, uint32_t max_steps, const float* bg_color3_host,
                                           float* image, float* depth, float* weights_sum, uint32_t* stats,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    ngp_camera cam;
    const int rc = nvf_fill_camera(pose_host, intrinsics_host, H, W, cam);
    if (rc != NGP_OK) return rc;
    return nvf_render_frame("nav_render_frame_camera", field_host, prepared, nullptr, nullptr, &cam, H * W, W, aabb_host, min_near, bitfield, C, Hgrid,
                            dt_gamma, max_steps, bg_color3_host, image, depth, weights_sum, stats, workspace, workspace_bytes, stream);
}
