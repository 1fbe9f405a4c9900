// Which band queue a wave of the frame kernel draws its next tile from (render_fused.hip, rv_frame_loop's refill).  Written once for the kernel and
// for the host export ngp_render_band_pick_host, which the CPU tests drive; plain integers only.
//
// Every band that still has tiles gets a KEY, and the largest key wins:
//   1. a band of the wave's own XCD (band % 8 == xcd) before any other XCD's,
//   2. then the larger estimate of the band's NEXT tile (each band hands out its tiles by decreasing estimate, so this merges the XCD's bands into
//      one descending list: the tiles drawn last are the cheapest of the XCD's whole share, not those of its last band),
//   3. then the lower rank = (((band % 8) - xcd) mod 8) * (bands / 8) + band / 8: the order x, x + 8, x + 16, x + 24, x + 1, ... the bands were walked
//      in before there were estimates.  With all estimates equal the picks reproduce that walk exactly.
// Hysteresis: the own band the wave drew from last counts with h times its estimate (h >= 1, in 1/256), and wins ties: the wave leaves it only
// when another band's next tile EXCEEDS h times this one's.  h = 1 is the pure merge.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGP_BAND_HD __host__ __device__ __forceinline__
#else
#define NGP_BAND_HD inline
#endif

static constexpr uint32_t NGP_BAND_H_ONE = 256u;              // h in 1/256
static constexpr uint32_t NGP_BAND_H_MAX = 256u * 64u;        // est * h stays below 2^46

NGP_BAND_HD uint32_t ngp_band_rank(uint32_t band, uint32_t xcd, uint32_t n_bands) {
    return (((band & 7u) - xcd) & 7u) * (n_bands >> 3) + (band >> 3);
}
NGP_BAND_HD uint32_t ngp_band_of_rank(uint32_t rank, uint32_t xcd, uint32_t n_bands) {
    const uint32_t per = n_bands >> 3;
    return (((rank / per) + xcd) & 7u) + 8u * (rank % per);
}

// The key of a band that has tiles left (a dry or empty band has key 0 and is never chosen).  is_last: the wave drew its previous tile from this band.
// Bits: 53 has tiles | 52 own XCD | 6..51 estimate x h | 5 the last band (wins a tie) | 0..4 31 - rank.
NGP_BAND_HD unsigned long long ngp_band_key(uint32_t band, uint32_t xcd, uint32_t n_bands, uint32_t estimate, bool is_last, uint32_t h_q8) {
    const bool own = (band & 7u) == xcd;
    const bool stay = is_last && own;
    const unsigned long long e = (unsigned long long)estimate * (stay ? h_q8 : NGP_BAND_H_ONE);
    return (1ull << 53) | ((unsigned long long)(own ? 1u : 0u) << 52) | (e << 6) | ((unsigned long long)(stay ? 1u : 0u) << 5) |
           (unsigned long long)(31u - ngp_band_rank(band, xcd, n_bands));
}
NGP_BAND_HD unsigned long long ngp_band_better(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
// the band of the winning key, or -1 when no band has tiles left
NGP_BAND_HD int ngp_band_of_key(unsigned long long key, uint32_t xcd, uint32_t n_bands) {
    return key ? (int)ngp_band_of_rank(31u - (uint32_t)(key & 31u), xcd, n_bands) : -1;
}

// Band b's rays [lo, hi) of a frame of n_rays rays in tiles of 64 (the last tile may be short).
NGP_BAND_HD void ngp_band_range(uint32_t n_rays, uint32_t band, uint32_t n_bands, uint32_t& lo, uint32_t& hi) {
    const uint32_t n_tiles64 = (uint32_t)(((unsigned long long)n_rays + 63u) >> 6);
    lo = (uint32_t)(((unsigned long long)n_tiles64 * band) / n_bands) << 6;
    hi = (uint32_t)(((unsigned long long)n_tiles64 * (band + 1u)) / n_bands) << 6;
    hi = hi < n_rays ? hi : n_rays;
}

// One band's look: `head` is what the wave read from the band's queue word (rays handed out; it only grows, so a stale value is too small, never too
// large).  Returns the key, 0 when the band has nothing left for this wave; *peek_dry is set when head or range say so, which is then true for good.
// perm / cost are read only for a band with tiles left: never for an empty band, whose lo may equal the number of tiles.
NGP_BAND_HD unsigned long long ngp_band_look(uint32_t band, uint32_t xcd, uint32_t n_bands, uint32_t n_rays, uint32_t head, uint32_t dry_mask, int last_band,
                                             uint32_t h_q8, const uint32_t* perm, const uint32_t* cost, bool* peek_dry) {
    *peek_dry = false;
    if ((dry_mask >> band) & 1u) return 0ull;
    uint32_t lo, hi;
    ngp_band_range(n_rays, band, n_bands, lo, hi);
    if (lo >= hi || head >= hi - lo) { *peek_dry = true; return 0ull; }
    const uint32_t estimate = (perm && cost) ? cost[perm[(lo + head) >> 6]] : 0u;
    return ngp_band_key(band, xcd, n_bands, estimate, (int)band == last_band, h_q8);
}
