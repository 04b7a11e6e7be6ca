// cups.hip -- suction cups of the layer stack on gfx950 (implisolid_layer_cups): for every layer l the empty
// voxels of layer l that belong to a pocket of the prefix 0 .. l (the connected empty voxels of layers 0 .. l under
// 6- or 26-adjacency) without a voxel on the image frame.  The plate below layer 0 and the film above layer l are
// closed, so only the frame lets a pocket out.  The runs, their numbering and the union-find are bodies.hip's with
// target 0 (launch_body_count, launch_body_emit, launch_body_link), with one change made by the caller: the
// stack's runs are numbered from 1, and run 0 is the outside, parent[0] = 0.  The smaller index is always the
// parent, so a pocket is open iff its root is 0, and a closed pocket's root is its earliest run, whose first voxel
// has the pocket's smallest key.  Joins only ever add up as layers arrive: one linking pass over the stack,
// queried behind each layer, answers every prefix.
//
// Whole-stack device memory besides bodies.hip's runs, parent and rowoff (12 bytes a run, 4 a row):
//   rootat  int32 per run: the run's root in its own layer's prefix                        4 bytes a run
//   cup     int32 per run: the head run of its cup (the cup's smallest run of the layer),
//           or -1 where the run's pocket is open                                            4 bytes a run
//   first   uint32 per run, read at roots only: see k_cup_mark; the finish pass keeps a
//           head's ordinal there (ord)                                                      4 bytes a run
//   rec     int64 {seed, area, x0, y0, x1, y1, pocket} per cup                             56 bytes a cup
//   out     int32 {start, length, cup} per cupped run, with want_runs                      12 bytes a cupped run
// and two counts and two scanned offsets per image row (16 bytes a row).  Nothing is per pixel.
//
// Per chunk, behind bodies.hip's count and emit:
// k_cup_frame : one wave per image row of the chunk, lanes over its runs: a run that holds a frame voxel (x0 == 0,
//               x1 == W - 1, or py 0 or H - 1) gets parent = 0.  A plain store: emit has just written parent = own
//               index, and no link pass has reached these layers.
// Then layer by layer on the stream, behind launch_body_link of that one layer:
// k_cup_mark  : a lane per run i of layer l, whose runs are [lo, hi): rootat[i] = its root r, found without
//               compressing paths, and for r != 0 atomicMax(first[r], lo + hi - 1 - i).  The values of a layer lie
//               in [lo, hi), above every earlier layer's, and the largest is the smallest run: first is zeroed
//               once and needs no reset between layers.
// k_cup_head  : cup[i] = lo + hi - 1 - first[rootat[i]], or -1 where rootat[i] == 0.
// The stream keeps layer l + 1's joins behind layer l's reads.  Behind the last chunk, over the whole stack:
// k_cup_rows  : one wave per four image rows in turn: the row's heads (cup[i] == i) and its cupped runs (cup[i] >=
//               0) by ballot, the block's cupped voxels onto the state with one atomic.
// k_cup_heads : one wave per image row: a head's ordinal is the row's offset (the exclusive scan of the head
//               counts) plus the heads in front of it in the row; run order is (layer, seed) order.  ord[head] =
//               ordinal, and the record is initialised {py W + x0, 0, MAX, MAX, -1, -1, pocket}: the pocket's key
//               is the row of rootat[head], bisected in rowoff, times W plus that run's x0.
// k_cup_tally : one wave per four image rows in turn, lanes over a row's runs: a cupped run adds its length and
//               extent to its head's record with 64-bit atomic add, min and max, folded over the wave where the
//               runs of a step share a cup as k_body_tally folds, and with want_runs stores {py W + x0, length,
//               ordinal} at the row's offset (the exclusive scan of the cupped-run counts) plus the cupped runs in
//               front of it in the row.
// No kernel waits for another block.  Every loop is bounded by the input: the walks by a row's runs; a find walks
// strictly decreasing indices and ends after at most `index` steps (unionfind_device.hpp); a bisection takes at
// most 32 rounds.  Everything is an integer: the results depend on no order of the atomics.
#include <climits>
#include <stdexcept>

#include "kernels.hpp"
#include "layer_device.hpp"
#include "unionfind_device.hpp"   // find_glb

namespace impli {

namespace {

constexpr uint32_t kRowsPerWave = 4;   // as bodies.hip's count and tally: a wave's rows share its atomics
constexpr uint32_t kNoCup = 0xffffffffu;

__global__ __launch_bounds__(256) void k_cup_frame(BodyGrid g, uint32_t rows, uint32_t row0, const int32_t* __restrict__ runs,
                                                   const uint32_t* __restrict__ rowoff, int32_t* __restrict__ parent) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const uint32_t Rg = row0 + R;
    const int py = (int)(Rg % (uint32_t)g.H);
    const bool edge = py == 0 || py == g.H - 1;
    const uint32_t lo = rowoff[Rg], hi = rowoff[(size_t)Rg + 1u];
    for (uint32_t i = lo + (uint32_t)lane; i < hi; i += 64u)
        if (edge || runs[2 * (size_t)i] == 0 || runs[2 * (size_t)i + 1] == g.W - 1) parent[i] = 0;
}

__global__ __launch_bounds__(256) void k_cup_mark(uint32_t lo, uint32_t hi, int32_t* parent, int32_t* __restrict__ rootat,
                                                  uint32_t* first) {
    const uint32_t i = lo + blockIdx.x * 256u + threadIdx.x;
    if (i >= hi) return;
    const int r = find_glb(parent, (int)i);   // 0 <= r <= i
    rootat[i] = r;
    if (r) atomicMax(&first[r], lo + hi - 1u - i);
}

__global__ __launch_bounds__(256) void k_cup_head(uint32_t lo, uint32_t hi, const int32_t* __restrict__ rootat,
                                                  const uint32_t* __restrict__ first, int32_t* __restrict__ cup) {
    const uint32_t i = lo + blockIdx.x * 256u + threadIdx.x;
    if (i >= hi) return;
    const int r = rootat[i];
    cup[i] = r ? (int32_t)(lo + hi - 1u - first[r]) : -1;   // first[r] in [lo, hi): run i itself has marked it
}

__global__ __launch_bounds__(256) void k_cup_rows(uint32_t rows, const int32_t* __restrict__ runs, const uint32_t* __restrict__ rowoff,
                                                  const int32_t* __restrict__ cup, uint32_t* __restrict__ head_counts,
                                                  uint32_t* __restrict__ run_counts, CupState* __restrict__ st) {
    __shared__ uint32_t s_vox[4];
    const int lane = threadIdx.x & 63;
    const uint32_t first = (blockIdx.x * 4u + (threadIdx.x >> 6)) * kRowsPerWave;   // wave-uniform
    uint32_t vox = 0;   // the lane's: <= 4 rows of 16384 pixels
    for (uint32_t k = 0; k < kRowsPerWave && first + k < rows; ++k) {
        const uint32_t R = first + k;
        const uint32_t lo = rowoff[R], hi = rowoff[(size_t)R + 1u];
        uint32_t nh = 0, nr = 0;
        for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {   // wave-uniform
            const uint32_t i = i0 + (uint32_t)lane;
            const int c = i < hi ? cup[i] : -1;
            nh += (uint32_t)__popcll((u64)__ballot(c == (int)i));
            nr += (uint32_t)__popcll((u64)__ballot(c >= 0));
            if (c >= 0) vox += (uint32_t)(runs[2 * (size_t)i + 1] - runs[2 * (size_t)i] + 1);
        }
        if (lane == 0) {
            head_counts[R] = nh;
            run_counts[R] = nr;
        }
    }
    wave_put(s_vox, wave_sum(vox));
    __syncthreads();   // every lane of the block arrives: no lane has returned
    if (threadIdx.x == 0) {
        const uint32_t total = block_sum(s_vox);   // <= 16 rows of 16384 pixels
        if (total) atomicAdd(&st->cupped, (u64)total);
    }
}

__global__ __launch_bounds__(256) void k_cup_heads(BodyGrid g, uint32_t rows, const int32_t* __restrict__ runs,
                                                   const uint32_t* __restrict__ rowoff, const int32_t* __restrict__ cup,
                                                   const int32_t* __restrict__ rootat, const uint32_t* __restrict__ offsets, uint32_t total,
                                                   uint32_t* __restrict__ ord, long long* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const long long py = (long long)(R % (uint32_t)g.H);
    const uint32_t lo = rowoff[R], hi = rowoff[(size_t)R + 1u];
    uint32_t base = offsets[R];
    for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {   // wave-uniform
        const uint32_t i = i0 + (uint32_t)lane;
        const bool head = i < hi && cup[i] == (int32_t)i;
        const u64 m = __ballot(head);
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (head && at < total) {   // at < total always: the scan counted these heads
            const uint32_t root = (uint32_t)rootat[i];   // in [1, i]: a head's pocket is closed
            uint32_t a = 0, b = R + 1u;   // rowoff[a] <= root < rowoff[b]: root <= i < rowoff[R + 1]
            while (b - a > 1u) {          // at most 32 rounds
                const uint32_t mid = a + (b - a) / 2u;
                if (rowoff[mid] <= root) a = mid;
                else b = mid;
            }
            ord[i] = at;
            long long* r = rec + 7 * (size_t)at;
            r[0] = py * g.W + runs[2 * (size_t)i];   // the head is the cup's first run of the layer
            r[1] = 0;
            r[2] = LLONG_MAX;
            r[3] = LLONG_MAX;
            r[4] = -1;
            r[5] = -1;
            r[6] = (long long)a * g.W + runs[2 * (size_t)root];   // a = l' H + py': the key of the root's first voxel
        }
        base += (uint32_t)__popcll(m);
    }
}

// voxels and an extent onto a cup's record
__device__ __forceinline__ void cup_add(long long* r, long long len, int x0, int x1, int y0, int y1) {
    __hip_atomic_fetch_add(r + 1, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rec_min(r + 2, x0);
    rec_min(r + 3, y0);
    rec_max(r + 4, x1);
    rec_max(r + 5, y1);
}

__global__ __launch_bounds__(256) void k_cup_tally(BodyGrid g, uint32_t rows, uint32_t end, const int32_t* __restrict__ runs,
                                                   const uint32_t* __restrict__ rowoff, const int32_t* __restrict__ cup,
                                                   const uint32_t* __restrict__ ord, uint32_t n_cups, long long* rec,
                                                   const uint32_t* __restrict__ offsets, uint32_t n_out, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t first = (blockIdx.x * 4u + (threadIdx.x >> 6)) * kRowsPerWave;   // wave-uniform
    // what the wave has gathered for one cup and not yet added to its record; all wave-uniform
    uint32_t cur = kNoCup;
    long long csum = 0;
    int cx0 = INT_MAX, cx1 = -1, cy0 = INT_MAX, cy1 = -1;
    for (uint32_t k = 0; k < kRowsPerWave && first + k < rows; ++k) {
        const uint32_t R = first + k;
        const int py = (int)(R % (uint32_t)g.H);
        const uint32_t lo = rowoff[R], hi = rowoff[(size_t)R + 1u];
        uint32_t base = offsets[R];   // the row's first cupped run in the output
        for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {   // wave-uniform
            const uint32_t i = i0 + (uint32_t)lane;
            const bool in = i < hi;
            int x0 = INT_MAX, x1 = -1, len = 0;
            uint32_t b = kNoCup;
            if (in) {
                const int c = cup[i];
                if (c >= 0 && (uint32_t)c < end) {   // c < end always: a head is a run of the stack
                    x0 = runs[2 * (size_t)i];
                    x1 = runs[2 * (size_t)i + 1];
                    len = x1 - x0 + 1;
                    b = ord[c];
                }
            }
            const bool cupped = b < n_cups;   // b != kNoCup: every head has an ordinal
            const u64 m = __ballot(cupped);
            if (m == 0ull) continue;          // wave-uniform
            if (out && cupped) {
                const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (at < n_out) {   // always: the scan counted these runs
                    int32_t* o = out + 3 * (size_t)at;
                    o[0] = py * g.W + x0;
                    o[1] = len;
                    o[2] = (int32_t)b;
                }
            }
            base += (uint32_t)__popcll(m);
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);   // lane 0 of the step always holds a run
            if (__ballot(in && b != b0) == 0ull) {
                // one cup for the whole step: the lengths and the extent fold over the wave and join what is gathered
                long long sum = len;
                int mn = x0, mx = x1;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    sum += __shfl_xor(sum, o, 64);
                    mn = min(mn, __shfl_xor(mn, o, 64));
                    mx = max(mx, __shfl_xor(mx, o, 64));
                }
                if (b0 != cur) {
                    if (lane == 0 && cur < n_cups) cup_add(rec + 7 * (size_t)cur, csum, cx0, cx1, cy0, cy1);
                    cur = b0;
                    csum = 0;
                    cx0 = cy0 = INT_MAX;
                    cx1 = cy1 = -1;
                }
                csum += sum;
                cx0 = min(cx0, mn);
                cx1 = max(cx1, mx);
                cy0 = min(cy0, py);
                cy1 = max(cy1, py);
            } else if (cupped) {
                cup_add(rec + 7 * (size_t)b, len, x0, x1, py, py);
            }
        }
    }
    if (lane == 0 && cur < n_cups) cup_add(rec + 7 * (size_t)cur, csum, cx0, cx1, cy0, cy1);
}

void check(const BodyGrid& g) {
    check_layer_chunk(g, 1u, "cups", "grid out of range");
    if (g.threshold < 1 || g.threshold > 16 || g.target != 0 || (g.connectivity != 6 && g.connectivity != 26))
        throw std::runtime_error("cups: grid out of range");
}
void check_stack(const BodyGrid& g, uint32_t rows) {
    check(g);
    if (rows < 1u || rows > kBodyMaxRows || rows % (uint32_t)g.H != 0u) throw std::runtime_error("cups: stack out of range");
}
// the runs [lo, hi) of one layer, numbered from 1
uint32_t check_layer_runs(uint32_t lo, uint32_t hi) {
    if (lo < 1u || hi < lo || hi > (1u << 31)) throw std::runtime_error("cups: run index out of range");
    return (hi - lo + 255u) / 256u;
}

}  // namespace

void launch_cup_frame(BodyGrid g, uint32_t n_layers, int l0, const int32_t* d_runs, const uint32_t* d_rowoff, int32_t* d_parent,
                      hipStream_t s) {
    check(g);
    check_layer_chunk(g, n_layers, "cups");
    if (l0 < 0 || ((uint64_t)l0 + n_layers) * (uint64_t)g.H > kBodyMaxRows) throw std::runtime_error("cups: chunk out of range");
    const uint32_t rows = n_layers * (uint32_t)g.H;
    k_cup_frame<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, (uint32_t)l0 * (uint32_t)g.H, d_runs, d_rowoff, d_parent);
}

void launch_cup_mark(uint32_t lo, uint32_t hi, int32_t* d_parent, int32_t* d_rootat, uint32_t* d_first, hipStream_t s) {
    const uint32_t blocks = check_layer_runs(lo, hi);
    if (blocks) k_cup_mark<<<blocks, 256, 0, s>>>(lo, hi, d_parent, d_rootat, d_first);
}

void launch_cup_head(uint32_t lo, uint32_t hi, const int32_t* d_rootat, const uint32_t* d_first, int32_t* d_cup, hipStream_t s) {
    const uint32_t blocks = check_layer_runs(lo, hi);
    if (blocks) k_cup_head<<<blocks, 256, 0, s>>>(lo, hi, d_rootat, d_first, d_cup);
}

void launch_cup_rows(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_cup,
                     uint32_t* d_head_counts, uint32_t* d_run_counts, CupState* d_state, hipStream_t s) {
    check_stack(g, rows);
    k_cup_rows<<<(rows + 4u * kRowsPerWave - 1u) / (4u * kRowsPerWave), 256, 0, s>>>(rows, d_runs, d_rowoff, d_cup, d_head_counts,
                                                                                    d_run_counts, d_state);
}

void launch_cup_heads(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_cup,
                      const int32_t* d_rootat, const uint32_t* d_offsets, uint32_t total, uint32_t* d_ord, long long* d_rec,
                      hipStream_t s) {
    check_stack(g, rows);
    if (total == 0u) return;
    k_cup_heads<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, d_runs, d_rowoff, d_cup, d_rootat, d_offsets, total, d_ord, d_rec);
}

void launch_cup_tally(BodyGrid g, uint32_t rows, uint32_t end, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_cup,
                      const uint32_t* d_ord, uint32_t n_cups, long long* d_rec, const uint32_t* d_offsets, uint32_t n_out,
                      int32_t* d_out, hipStream_t s) {
    check_stack(g, rows);
    if (n_cups == 0u) return;
    k_cup_tally<<<(rows + 4u * kRowsPerWave - 1u) / (4u * kRowsPerWave), 256, 0, s>>>(g, rows, end, d_runs, d_rowoff, d_cup, d_ord, n_cups,
                                                                                     d_rec, d_offsets, n_out, d_out);
}

}  // namespace impli
