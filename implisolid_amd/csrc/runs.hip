// runs.hip -- run-length layer images on gfx950 (implisolid_layer_runs): every layer of a chunk's image as
// the runs of its row-major pixel stream p = py W + px over the W real pixels of each row.  The chunk's image
// is raster.hip's (H rows of `pitch` = 16 ntx bytes per layer, padding columns zero, layers back to back);
// a pixel's value is its coverage byte (threshold 0) or cov >= threshold as 0 / 1.  A run starts at p = 0 and
// wherever the value differs from the pixel before in the stream, which for px = 0 is the last real pixel
// W - 1 of the row above: it sits at (py - 1) pitch + W - 1, not in front of the row's first byte.
//
// k_run_count : one wave per image row, 256 pixels a step: a lane loads one aligned dword, its four pixels.
//               A lane's predecessor is its neighbour lane's last pixel; lane 0 takes the last pixel of the
//               step before (a lane read), and in the first step the pixel W - 1 of the row above (none for
//               py = 0: p = 0 always starts a run).  Four ballots of "starts a run", one per byte of the
//               dword, and their popcounts add up in a register; one store per row.
// k_run_emit  : the same walk.  A start's ordinal is the row's offset (the exclusive scan of the counts) plus
//               the row's running count plus the starts in the lanes below plus the starts in front of it in
//               its own lane; there it stores the start's p and value.  Rows ascend with p and the scan
//               follows the rows, so the records are in increasing start by construction.
// No kernel waits for another block; both loops are bounded by W; there is no atomic.
#include <stdexcept>

#include "kernels.hpp"
#include "layer_device.hpp"

namespace impli {

namespace {

// the four pixel values of a dword of coverage bytes, byte for byte
__device__ __forceinline__ uint32_t run_values(uint32_t cov4, int threshold) {
    if (threshold == 0) return cov4;
    const uint32_t s = cov_solid4(cov4, threshold);
    return (s & 1u) | ((s & 2u) << 7) | ((s & 4u) << 14) | ((s & 8u) << 21);   // bit k into byte k
}

// One step of a row's walk: the pixels [x0, x0 + 256) of row R, four per lane.  v: the lane's four values;
// returns the lane's four "starts a run" flags (bit k: pixel x0 + 4 lane + k).  carry: in, the value in front
// of pixel x0 (not used for x0 == 0 of a layer's first row); out, the value of pixel x0 + 255.
__device__ __forceinline__ uint32_t run_step(const LayerGrid& g, const uint8_t* __restrict__ row, int py, int x0, int lane,
                                             uint32_t& carry, uint32_t& v) {
    const int px = x0 + 4 * lane;
    v = run_values(cov_load4(row + px, (uint32_t)px < g.pitch), g.threshold);   // pitch % 16 == 0: px + 3 < pitch
    const uint32_t up = (uint32_t)__shfl_up((int)v, 1, 64) >> 24;
    const uint32_t before = (v << 8) | (lane ? up : carry);
    const uint32_t diff = v ^ before;
    uint32_t starts = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool first = py == 0 && px + k == 0;   // p = 0: no pixel before it
        const bool s = px + k < g.W && (first || ((diff >> (8 * k)) & 0xffu) != 0u);
        starts |= (uint32_t)s << k;
    }
    carry = (uint32_t)__builtin_amdgcn_readlane((int)v, 63) >> 24;
    return starts;
}

// the value in front of a row's first pixel: pixel W - 1 of the row above, a pitched address (py > 0)
__device__ __forceinline__ uint32_t run_row_carry(const LayerGrid& g, const uint8_t* __restrict__ row, int py) {
    if (py == 0) return 0u;
    const uint32_t c = row[(ptrdiff_t)(g.W - 1) - (ptrdiff_t)g.pitch];
    return g.threshold ? (uint32_t)((int)c >= g.threshold) : c;
}

__global__ __launch_bounds__(256) void k_run_count(LayerGrid g, uint32_t rows, const uint8_t* __restrict__ img,
                                                   uint32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);   // wave-uniform
    if (R >= rows) return;
    const int py = (int)(R % (uint32_t)g.H);
    const uint8_t* row = img + (size_t)R * g.pitch;
    uint32_t carry = run_row_carry(g, row, py), cnt = 0, v;
    for (int x0 = 0; x0 < g.W; x0 += 256) {
        const uint32_t starts = run_step(g, row, py, x0, lane, carry, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt += (uint32_t)__popcll((u64)__ballot((starts >> k) & 1u));
    }
    if (lane == 0) counts[R] = cnt;
}

__global__ __launch_bounds__(256) void k_run_emit(LayerGrid g, uint32_t rows, const uint8_t* __restrict__ img,
                                                  const uint32_t* __restrict__ offsets, uint32_t total,
                                                  uint32_t* __restrict__ start, uint8_t* __restrict__ value) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const int py = (int)(R % (uint32_t)g.H);
    const uint8_t* row = img + (size_t)R * g.pitch;
    uint32_t carry = run_row_carry(g, row, py), v;
    uint32_t base = offsets[R];   // the row's offset, then the row's running count on top of it
    for (int x0 = 0; x0 < g.W; x0 += 256) {
        const uint32_t starts = run_step(g, row, py, x0, lane, carry, v);
        uint32_t step;
        uint32_t at = base + ranks_below(starts, step);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if ((starts >> k) & 1u) {
                if (at < total) {   // always: the scan counted these starts
                    start[at] = (uint32_t)py * (uint32_t)g.W + (uint32_t)(x0 + 4 * lane + k);   // < W H <= 2^28
                    value[at] = (uint8_t)(v >> (8 * k));
                }
                ++at;
            }
        }
        base += step;
    }
}

void check(const LayerGrid& g, uint32_t n_layers) {
    check_layer_chunk(g, n_layers, "runs");
    if (g.threshold < 0 || g.threshold > 16) throw std::runtime_error("runs: chunk out of range");   // 0: the value is the coverage byte
}

}  // namespace

void launch_run_count(LayerGrid g, uint32_t n_layers, const uint8_t* d_img, uint32_t* d_counts, hipStream_t s) {
    check(g, n_layers);
    const uint32_t rows = n_layers * (uint32_t)g.H;   // <= 2^28
    k_run_count<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, d_img, d_counts);
}

void launch_run_emit(LayerGrid g, uint32_t n_layers, const uint8_t* d_img, const uint32_t* d_offsets, uint32_t total,
                     uint32_t* d_start, uint8_t* d_value, hipStream_t s) {
    check(g, n_layers);
    if (total == 0u) return;
    const uint32_t rows = n_layers * (uint32_t)g.H;
    k_run_emit<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, d_img, d_offsets, total, d_start, d_value);
}

}  // namespace impli
