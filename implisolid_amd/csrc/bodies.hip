// bodies.hip -- connected components of the layer stack on gfx950 (implisolid_layer_bodies): the classes of
// the target voxels (solid: cov >= threshold, or empty: cov < threshold) under 6- or 26-adjacency through the
// whole stack, as a union-find over the stack's row runs.  A row run is a maximal sequence of target voxels
// inside one image row (l, py); the runs are numbered layer by layer, row by row, left to right, which is the
// order of their first voxels' keys l W H + py W + px.  The chunk's image is raster.hip's (H rows of `pitch`
// = 16 ntx bytes per layer, padding columns zero, layers back to back); nothing else is per pixel.
//
// Whole-stack device memory, kept from the first chunk to the download:
//   runs    int32 {x0, x1} per run, inclusive                         8 bytes a run
//   parent  int32 per run, the union-find                             4 bytes a run
//   ord     uint32 per run, a root's body ordinal (finish only)       4 bytes a run
//   out     int32 {start, length, body} per run, with want_runs      12 bytes a run
//   rowoff  uint32 per image row of the stack, + 1: row (l, py)'s runs are [rowoff[l H + py], rowoff[l H + py + 1]);
//           the finish pass adds a count and a scanned offset per row 12 bytes a row
//   rec     int64 {seed, volume, x0, y0, l0, x1, y1, l1} per body    64 bytes a body
// that is 16 bytes a run, 28 with want_runs.
//
// k_body_count : one wave per four image rows in turn, 256 pixels a step: a lane loads one aligned dword, its
//                four pixels, and makes the four "is of the target class" bits (false at and past pixel W).  A run starts where
//                a bit is set and the pixel before is not (a lane's predecessor is its neighbour lane's last
//                pixel, lane 0 takes the last pixel of the step before, and nothing stands in front of pixel
//                0).  Four ballots of "starts a run" and four of the bits; the row's run count in one store,
//                the block's target voxels (sixteen rows) onto the state with one atomic.
// k_body_emit  : the same walk.  A start's ordinal is the row's offset plus the row's running count plus the
//                starts in the lanes below plus the starts in front of it in its own lane; there it stores x0
//                and parent = own index.  A run ends in front of the first pixel that is not of the class
//                behind one that is; the k-th end of a row closes its k-th start, so x1 is stored by the same
//                rule.  Pixel W ends a run like any other unless W is a multiple of 256: then the row's last
//                run, if it reaches W - 1, is closed behind the loop.  The row's offset goes into rowoff.
// k_body_link  : one wave per image row, lanes over the row's runs (a loop where a row has more than 64).  For
//                every neighbour row -- (l, py - 1) and (l - 1, py) with d = 0 under connectivity 6; (l, py - 1),
//                (l - 1, py - 1), (l - 1, py), (l - 1, py + 1) with d = 1 under 26 -- the run bisects that row's
//                runs for the first with x1 >= x0 - d and walks on while x0' <= x1 + d, uniting as it goes.
//                The rows of the layer below a chunk's first layer are read from the stack's arrays.
// k_body_root_rows : one wave per image row of the stack: its roots (parent == own index), by ballot.
// k_body_roots : the same walk: a root's ordinal is the row's offset (the exclusive scan of the counts) plus
//                the roots in front of it in the row; ord[run] = ordinal, and the record is initialised {key of
//                its first voxel, 0, INT64_MAX, INT64_MAX, l, -1, -1, -1}.  Run order is key order, so the roots in
//                run order are the bodies in seed order.
// k_body_tally : one wave per four image rows in turn, lanes over a row's runs: find the root, take its ordinal,
//                add the run's length and extent to the record with 64-bit atomic add, min and max, and with
//                want_runs store {py W + x0, length, ordinal}.  Where the runs of a step share a body they fold
//                over the wave, and the wave gathers as long as the body stays the same: one add per body and
//                wave in the usual case.  A min or max that would not change its field is left out.
// No kernel waits for another block.  Every loop is bounded by the input: the walks by W or by a row's runs;
// a find walks strictly decreasing indices, and in a union the larger of the two indices strictly decreases
// from round to round (unionfind_device.hpp), so both end after at most `index` steps; a bisection takes at
// most 32 rounds.  Everything is an integer: the results depend on no order of the atomics.
#include <climits>
#include <stdexcept>

#include "kernels.hpp"
#include "layer_device.hpp"
#include "unionfind_device.hpp"   // find_glb, unite<>

namespace impli {

namespace {

// One step of a row's walk: the pixels [x0, x0 + 256), four per lane.  t: the lane's four class bits (bit k: pixel
// x0 + 4 lane + k is of the target class; 0 at and past pixel W); returns the lane's four "starts a run" bits and
// in `fall` its four "is not of the class, the pixel before is" bits.  carry: in, the class bit of pixel x0 - 1 (0
// for x0 == 0); out, that of pixel x0 + 255.
__device__ __forceinline__ uint32_t body_step(const BodyGrid& g, const uint8_t* __restrict__ row, int x0, int lane, uint32_t& carry,
                                              uint32_t& t, uint32_t& fall) {
    const int px = x0 + 4 * lane;
    const uint32_t cov4 = cov_load4(row + px, (uint32_t)px < g.pitch);   // pitch % 16 == 0: px + 3 < pitch
    t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool solid = cov_solid(cov4, (uint32_t)k, g.threshold);
        t |= (uint32_t)(px + k < g.W && solid == (g.target != 0)) << k;
    }
    const uint32_t up = ((uint32_t)__shfl_up((int)t, 1, 64) >> 3) & 1u;
    const uint32_t before = ((t << 1) | (lane ? up : carry)) & 15u;
    fall = ~t & before;
    carry = ((uint32_t)__builtin_amdgcn_readlane((int)t, 63) >> 3) & 1u;
    return t & ~before;
}

// rows a wave of the count and tally passes takes in turn: their sums reach the state and the records with one
// atomic where a wave a row would issue four
constexpr uint32_t kRowsPerWave = 4;

__global__ __launch_bounds__(256) void k_body_count(BodyGrid g, uint32_t rows, const uint8_t* __restrict__ img,
                                                    uint32_t* __restrict__ counts, BodyState* __restrict__ st) {
    __shared__ uint32_t s_vox[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t first = (blockIdx.x * 4u + (uint32_t)wv) * kRowsPerWave;   // wave-uniform
    uint32_t vox = 0;   // <= 4 rows of 16384 pixels
    for (uint32_t k = 0; k < kRowsPerWave && first + k < rows; ++k) {
        const uint32_t R = first + k;
        const uint8_t* row = img + (size_t)R * g.pitch;
        uint32_t carry = 0, cnt = 0, t, fall;
        for (int x0 = 0; x0 < g.W; x0 += 256) {
            const uint32_t rise = body_step(g, row, x0, lane, carry, t, fall);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                cnt += (uint32_t)__popcll((u64)__ballot((rise >> b) & 1u));
                vox += (uint32_t)__popcll((u64)__ballot((t >> b) & 1u));
            }
        }
        if (lane == 0) counts[R] = cnt;
    }
    wave_put(s_vox, vox);
    __syncthreads();   // every lane of the block arrives: no lane has returned
    if (threadIdx.x == 0) {
        const uint32_t total = block_sum(s_vox);
        if (total) atomicAdd(&st->voxels, (u64)total);
    }
}

__global__ __launch_bounds__(256) void k_body_emit(BodyGrid g, uint32_t rows, uint32_t row0, const uint8_t* __restrict__ img,
                                                   const uint32_t* __restrict__ offsets, uint32_t base, uint32_t end,
                                                   int32_t* __restrict__ runs, int32_t* __restrict__ parent, uint32_t* __restrict__ rowoff) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const uint8_t* row = img + (size_t)R * g.pitch;
    const uint32_t first = base + offsets[R];   // the row's first run in the stack's numbering
    if (lane == 0) {
        rowoff[(size_t)row0 + R] = first;
        if (R + 1u == rows) rowoff[(size_t)row0 + rows] = base + offsets[rows];   // the next chunk's first row stores the same
    }
    uint32_t carry = 0, t, fall, nr = first, nf = first;   // the ordinals of the step's first start and first end
    for (int x0 = 0; x0 < g.W; x0 += 256) {
        const uint32_t rise = body_step(g, row, x0, lane, carry, t, fall);
        uint32_t all_r, all_f;
        uint32_t at = nr + ranks_below(rise, all_r), af = nf + ranks_below(fall, all_f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int px = x0 + 4 * lane + k;
            if ((rise >> k) & 1u) {
                if (at < end) {   // always: the scan counted these starts
                    runs[2 * (size_t)at] = px;
                    parent[at] = (int32_t)at;
                }
                ++at;
            }
            if ((fall >> k) & 1u) {
                if (af < end) runs[2 * (size_t)af + 1] = px - 1;   // af < at: every end closes a start in front of it
                ++af;
            }
        }
        nr += all_r;
        nf += all_f;
    }
    // W % 256 == 0 and the last pixel is of the class: no pixel of the walk stood behind the row's last run
    if (carry && lane == 0 && nf < end) runs[2 * (size_t)nf + 1] = g.W - 1;
}

// joins run i = {x0, x1} with the runs of row Rn that reach into [x0 - d, x1 + d]
__device__ __forceinline__ void link_row(const int32_t* __restrict__ runs, const uint32_t* __restrict__ rowoff, int32_t* parent,
                                         uint32_t Rn, uint32_t i, int x0, int x1, int d) {
    uint32_t lo = rowoff[Rn], hi = rowoff[(size_t)Rn + 1u];
    const uint32_t end = hi;
    while (lo < hi) {   // at most 32 rounds: the first run with x1' >= x0 - d
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (runs[2 * (size_t)mid + 1] < x0 - d) lo = mid + 1u;
        else hi = mid;
    }
    for (uint32_t j = lo; j < end && runs[2 * (size_t)j] <= x1 + d; ++j) unite<false>(parent, (int)i, (int)j);
}

__global__ __launch_bounds__(256) void k_body_link(BodyGrid g, uint32_t rows, uint32_t row0, const int32_t* __restrict__ runs,
                                                   const uint32_t* __restrict__ rowoff, int32_t* parent) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const uint32_t Rg = row0 + R, H = (uint32_t)g.H;   // the row in the stack: l H + py
    const int py = (int)(Rg % H);
    const bool below = Rg >= H, wide = g.connectivity == 26;
    const int d = wide ? 1 : 0;
    const uint32_t lo = rowoff[Rg], hi = rowoff[(size_t)Rg + 1u];
    for (uint32_t i = lo + (uint32_t)lane; i < hi; i += 64u) {
        const int x0 = runs[2 * (size_t)i], x1 = runs[2 * (size_t)i + 1];
        if (py > 0) link_row(runs, rowoff, parent, Rg - 1u, i, x0, x1, d);
        if (below) {
            if (wide && py > 0) link_row(runs, rowoff, parent, Rg - H - 1u, i, x0, x1, d);
            link_row(runs, rowoff, parent, Rg - H, i, x0, x1, d);
            if (wide && py + 1 < g.H) link_row(runs, rowoff, parent, Rg - H + 1u, i, x0, x1, d);
        }
    }
}

__global__ __launch_bounds__(256) void k_body_root_rows(uint32_t rows, const uint32_t* __restrict__ rowoff,
                                                        const int32_t* __restrict__ parent, uint32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const uint32_t lo = rowoff[R], hi = rowoff[(size_t)R + 1u];
    uint32_t cnt = 0;
    for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {   // wave-uniform
        const uint32_t i = i0 + (uint32_t)lane;
        const bool root = i < hi && parent[i] == (int32_t)i;
        cnt += (uint32_t)__popcll((u64)__ballot(root));
    }
    if (lane == 0) counts[R] = cnt;
}

__global__ __launch_bounds__(256) void k_body_roots(BodyGrid g, uint32_t rows, const int32_t* __restrict__ runs,
                                                    const uint32_t* __restrict__ rowoff, const int32_t* __restrict__ parent,
                                                    const uint32_t* __restrict__ offsets, uint32_t total, uint32_t* __restrict__ ord,
                                                    long long* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const long long l = (long long)(R / (uint32_t)g.H), py = (long long)(R % (uint32_t)g.H);
    const uint32_t lo = rowoff[R], hi = rowoff[(size_t)R + 1u];
    uint32_t base = offsets[R];
    for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {
        const uint32_t i = i0 + (uint32_t)lane;
        const bool root = i < hi && parent[i] == (int32_t)i;
        const u64 m = __ballot(root);
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (root && at < total) {   // at < total always: the scan counted these roots
            ord[i] = at;
            long long* r = rec + 8 * (size_t)at;
            r[0] = (l * g.H + py) * g.W + runs[2 * (size_t)i];   // the key of the body's first voxel
            r[1] = 0;
            r[2] = LLONG_MAX;
            r[3] = LLONG_MAX;
            r[4] = l;   // the seed is the smallest key: its layer is l0
            r[5] = -1;
            r[6] = -1;
            r[7] = -1;
        }
        base += (uint32_t)__popcll(m);
    }
}

// voxels and an extent onto a record; l0 is the seed's layer and was stored with the record
__device__ __forceinline__ void rec_add(long long* r, long long len, int x0, int x1, int y0, int y1, int l1) {
    __hip_atomic_fetch_add(r + 1, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rec_min(r + 2, x0);
    rec_min(r + 3, y0);
    rec_max(r + 5, x1);
    rec_max(r + 6, y1);
    rec_max(r + 7, l1);
}

__global__ __launch_bounds__(256) void k_body_tally(BodyGrid g, uint32_t rows, const int32_t* __restrict__ runs,
                                                    const uint32_t* __restrict__ rowoff, int32_t* parent, const uint32_t* __restrict__ ord,
                                                    uint32_t n_bodies, long long* rec, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t first = (blockIdx.x * 4u + (threadIdx.x >> 6)) * kRowsPerWave;   // wave-uniform
    // what the wave has gathered for one body and not yet added to its record; all wave-uniform
    uint32_t cur = 0xffffffffu;
    long long csum = 0;
    int cx0 = INT_MAX, cx1 = -1, cy0 = INT_MAX, cy1 = -1, cl1 = -1;
    for (uint32_t k = 0; k < kRowsPerWave && first + k < rows; ++k) {
        const uint32_t R = first + k;
        const int l = (int)(R / (uint32_t)g.H), py = (int)(R % (uint32_t)g.H);
        const uint32_t lo = rowoff[R], hi = rowoff[(size_t)R + 1u];
        for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {   // wave-uniform
            const uint32_t i = i0 + (uint32_t)lane;
            const bool in = i < hi;
            int x0 = INT_MAX, x1 = -1, len = 0;
            uint32_t b = 0;
            if (in) {
                x0 = runs[2 * (size_t)i];
                x1 = runs[2 * (size_t)i + 1];
                len = x1 - x0 + 1;
                b = ord[find_glb(parent, (int)i)];
                if (out && b < n_bodies) {
                    int32_t* o = out + 3 * (size_t)i;
                    o[0] = py * g.W + x0;
                    o[1] = len;
                    o[2] = (int32_t)b;
                }
            }
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);   // lane 0 of the step always holds a run
            if (__ballot(in && b != b0) == 0ull) {
                // one body for the whole step: the lengths and the extent fold over the wave and join what is gathered
                long long sum = len;
                int mn = x0, mx = x1;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    sum += __shfl_xor(sum, o, 64);
                    mn = min(mn, __shfl_xor(mn, o, 64));
                    mx = max(mx, __shfl_xor(mx, o, 64));
                }
                if (b0 != cur) {
                    if (lane == 0 && cur < n_bodies) rec_add(rec + 8 * (size_t)cur, csum, cx0, cx1, cy0, cy1, cl1);
                    cur = b0;
                    csum = 0;
                    cx0 = cy0 = INT_MAX;
                    cx1 = cy1 = cl1 = -1;
                }
                csum += sum;
                cx0 = min(cx0, mn);
                cx1 = max(cx1, mx);
                cy0 = min(cy0, py);
                cy1 = max(cy1, py);
                cl1 = max(cl1, l);
            } else if (in && b < n_bodies) {   // b < n_bodies always: every root has an ordinal
                rec_add(rec + 8 * (size_t)b, len, x0, x1, py, py, l);
            }
        }
    }
    if (lane == 0 && cur < n_bodies) rec_add(rec + 8 * (size_t)cur, csum, cx0, cx1, cy0, cy1, cl1);
}

void check(const BodyGrid& g) {
    check_layer_chunk(g, 1u, "bodies", "grid out of range");
    if (g.threshold < 1 || g.threshold > 16 || (g.target != 0 && g.target != 1) || (g.connectivity != 6 && g.connectivity != 26))
        throw std::runtime_error("bodies: grid out of range");
}
// a chunk's rows, and the rows of the stack in front of it
void check(const BodyGrid& g, uint32_t n_layers, int l0) {
    check(g);
    check_layer_chunk(g, n_layers, "bodies");
    if (l0 < 0 || ((uint64_t)l0 + n_layers) * (uint64_t)g.H > kBodyMaxRows) throw std::runtime_error("bodies: chunk out of range");
}
void check_stack(const BodyGrid& g, uint32_t rows) {
    check(g);
    if (rows < 1u || rows > kBodyMaxRows || rows % (uint32_t)g.H != 0u) throw std::runtime_error("bodies: stack out of range");
}

}  // namespace

void launch_body_count(BodyGrid g, uint32_t n_layers, const uint8_t* d_img, uint32_t* d_counts, BodyState* d_state, hipStream_t s) {
    check(g, n_layers, 0);
    const uint32_t rows = n_layers * (uint32_t)g.H;   // <= 2^28
    k_body_count<<<(rows + 4u * kRowsPerWave - 1u) / (4u * kRowsPerWave), 256, 0, s>>>(g, rows, d_img, d_counts, d_state);
}

void launch_body_emit(BodyGrid g, uint32_t n_layers, int l0, const uint8_t* d_img, const uint32_t* d_offsets, uint32_t base,
                      uint32_t total, int32_t* d_runs, int32_t* d_parent, uint32_t* d_rowoff, hipStream_t s) {
    check(g, n_layers, l0);
    if ((uint64_t)base + total >= (1ull << 31)) throw std::runtime_error("bodies: run index out of range");
    const uint32_t rows = n_layers * (uint32_t)g.H;
    k_body_emit<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, (uint32_t)l0 * (uint32_t)g.H, d_img, d_offsets, base, base + total, d_runs,
                                                  d_parent, d_rowoff);
}

void launch_body_link(BodyGrid g, uint32_t n_layers, int l0, const int32_t* d_runs, const uint32_t* d_rowoff, int32_t* d_parent,
                      hipStream_t s) {
    check(g, n_layers, l0);
    const uint32_t rows = n_layers * (uint32_t)g.H;
    k_body_link<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, (uint32_t)l0 * (uint32_t)g.H, d_runs, d_rowoff, d_parent);
}

void launch_body_root_rows(BodyGrid g, uint32_t rows, const uint32_t* d_rowoff, const int32_t* d_parent, uint32_t* d_counts,
                           hipStream_t s) {
    check_stack(g, rows);
    k_body_root_rows<<<(rows + 3u) / 4u, 256, 0, s>>>(rows, d_rowoff, d_parent, d_counts);
}

void launch_body_roots(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_parent,
                       const uint32_t* d_offsets, uint32_t total, uint32_t* d_ord, long long* d_rec, hipStream_t s) {
    check_stack(g, rows);
    if (total == 0u) return;
    k_body_roots<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, d_runs, d_rowoff, d_parent, d_offsets, total, d_ord, d_rec);
}

void launch_body_tally(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, int32_t* d_parent,
                       const uint32_t* d_ord, uint32_t n_bodies, long long* d_rec, int32_t* d_out, hipStream_t s) {
    check_stack(g, rows);
    if (n_bodies == 0u) return;
    k_body_tally<<<(rows + 4u * kRowsPerWave - 1u) / (4u * kRowsPerWave), 256, 0, s>>>(g, rows, d_runs, d_rowoff, d_parent, d_ord, n_bodies, d_rec, d_out);
}

}  // namespace impli
