// rayspans.hip -- every solid span along a ray on gfx950 (implisolid_ray_spans): the maximal runs of solid
// samples (!(F < 0)) among the N + 1 samples ts[k] of p(t) = o + t d, each with its entry and its exit
// refined by B bisection rounds, the field there and the normals.  The sample table, the 64-step segments
// and the bound of a segment's box are raycast.hip's (ray_device.hpp holds what the two files share).
//
// k_span_march  : one wave per ray, four rays per block.  Lane i of a batch bounds segment j0 + i over the
//                 box of its two end points: hi < 0 proves every sample of it outside, lo >= 0 proves every
//                 sample solid (the box holds every p(t) of the segment, and a finite box only: a segment
//                 with an end point that is not finite is proved nothing).  The wave walks the others in
//                 order under their modes words; one ballot of the samples 64 j + 1 + lane is segment j's
//                 solidity word W (bit i = sample 64 j + 1 + i), which lane j - j0 keeps.  A proved
//                 segment's word is 0 or the mask of its samples.  Sample 0 belongs to segment 0: lane 0
//                 evaluates it in a pass of its own, or segment 0's proof decides it.  All segments but
//                 the last hold 64 samples, so the sample in front of segment j's first is bit 63 of word
//                 j - 1 (sample 0's state for j = 0), and the entries of a word are W & ~((W << 1) | prev).
//                 Per ray: the words, the span count (entries, plus one for a solid sample 0) and the
//                 proved segments.  The whole ray is walked: no early end.
// k_span_tally  : one lane per ray; the chunk's work figures, summed per wave, one atomic per counter.
// k_span_emit   : one wave per ray, after the scan of the counts.  Entries and exits alternate along a
//                 ray, so the i-th entry and the i-th exit are span i's: lanes take the words, a wave
//                 prefix of their entry and exit counts gives the ranks, and each lane writes the k_in and
//                 the k_out its word holds.  The bit behind the last sample of a partial last segment is
//                 an exit at N + 1 by the same formula; a full last segment that ends solid gets it from
//                 lane 0.  A span that opens in one segment or batch and closes in another needs no state.
// k_span_refine : one lane per span end.  The end's bracket lies in segment (k - 1) / 64, whose box is
//                 bounded again for the modes word (bit-identical values; a word per (ray, segment) would
//                 cost as much memory as the solidity words).  F at the solid end, then B rounds towards
//                 the other end, entries downwards and exits upwards; k_in = 0 and k_out = N + 1 have no
//                 bracket and keep ts[0] and ts[N].  The normal is vertex_normal_at's.
// No result depends on the pruning level, the chunks or the order of any atomic.
#include <stdexcept>

#include "ifunc_device.hpp"
#include "ifunc_interval.hpp"
#include "ob02_device.hpp"
#include "ray_device.hpp"
#include "kernels.hpp"

namespace impli {

using namespace dev;
using namespace ray;

namespace {

typedef unsigned long long u64;
constexpr int kSeg = kRaySegment;
static_assert(kSeg == 64, "one sample of a segment per lane, one bit of a word per sample");

// the bound of segment seg's box and its modes word (0 where an end point is not finite: proved nothing)
template <int D>
__device__ __forceinline__ Iv bound_segment(const Program* __restrict__ prog, const float* __restrict__ tab, float2 tab_range,
                                            const float* __restrict__ ts, const RayAt& ray, int seg, int N, uint64_t& m,
                                            bool& fin) {
    // ts[kSeg seg] and ts[min(kSeg seg + kSeg, N)]: indices within 0 .. N for seg < nseg
    const int k1 = min(kSeg * seg + kSeg, N);
    const V3 a = ray_point(ray, ts[kSeg * seg]), b = ray_point(ray, ts[k1]);
    const Iv iv = eval_iv<D>(prog, tab, tab_range, Box{span(a.x, b.x), span(a.y, b.y), span(a.z, b.z)}, 0ull, m);
    fin = finite3(a) && finite3(b);   // then every point between them is finite
    if (!fin) m = 0;
    return iv;
}

template <int D>
__global__ __launch_bounds__(256) void k_span_march(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                     float2 tab_range, const float* __restrict__ ts,
                                                     const float* __restrict__ org, const float* __restrict__ dir, uint32_t n,
                                                     int N, int prune, uint64_t* __restrict__ words,
                                                     uint32_t* __restrict__ counts, uint32_t* __restrict__ info) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t r = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= n) return;   // the whole wave: nothing below crosses waves
    const RayAt ray = ray_at(org, dir, r);
    const int nseg = (N + kSeg - 1) / kSeg;
    uint64_t* __restrict__ w_r = words + (size_t)r * (size_t)nseg;
    uint32_t rises = 0;                             // per lane, summed at the end
    uint32_t n_out = 0, n_solid = 0, s0 = 0, carry = 0;   // wave-uniform
    for (int j0 = 0; j0 < nseg; j0 += 64) {
        const int seg = j0 + lane;
        const bool valid = seg < nseg;
        uint64_t m = 0;
        bool outside = false, solid = false;
        if (prune && valid) {
            bool fin;
            const Iv iv = bound_segment<D>(prog, tab, tab_range, ts, ray, seg, N, m, fin);
            solid = fin && iv.lo >= 0.f;               // a NaN bound proves nothing
            outside = fin && !solid && iv.hi < 0.f;
        }
        const int nv = valid ? min(kSeg, N - kSeg * seg) : 0;   // the segment's samples: 1 .. 64
        uint64_t w = solid ? (nv >= 64 ? ~0ull : (1ull << nv) - 1ull) : 0ull;
        const uint64_t outm = (uint64_t)__ballot(valid && outside), solidm = (uint64_t)__ballot(valid && solid);
        uint64_t live = (uint64_t)__ballot(valid && !outside && !solid);
        n_out += (uint32_t)__popcll((u64)outm);
        n_solid += (uint32_t)__popcll((u64)solidm);
        if (j0 == 0) s0 = (uint32_t)(solidm & 1ull);   // segment 0 proved: its proof speaks of sample 0 too
        while (live) {
            const int q = __builtin_ctzll((u64)live);
            live &= live - 1ull;
            const uint64_t mq = wave_bcast(m, q);
            const int sg = j0 + q;
            // segment 0 holds sample 0 as well: lane 0 takes it in a pass of its own
            for (int pass = sg == 0 ? 0 : 1; pass < 2; ++pass) {
                const int k = pass == 0 ? 0 : kSeg * sg + 1 + lane;
                const bool has = pass == 0 ? lane == 0 : k <= N;
                float f = -1.f;
                if (has) {
                    const V3 p = ray_point(ray, ts[k]);
                    f = ray_field<D>(prog, tab, mq, p);
                }
                const uint64_t hm = (uint64_t)__ballot(has && !(f < 0.f));   // marching cubes' rule: -0.0 and NaN are solid
                if (pass == 0) s0 = (uint32_t)(hm & 1ull);
                else if (lane == q) w = hm;
            }
        }
        // the sample in front of the word's first: bit 63 of the word before (every segment but the last is full)
        const uint32_t top = (uint32_t)(w >> 63);
        uint32_t prev = (uint32_t)__shfl_up((int)top, 1, 64);
        if (lane == 0) prev = j0 == 0 ? s0 : carry;
        carry = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)top, 63, 64));
        rises += (uint32_t)__popcll((u64)(w & ~((w << 1) | (uint64_t)prev)));
        if (valid) w_r[seg] = w;
    }
    const uint32_t total = wave_sum(rises) + s0;
    if (lane == 0) {
        counts[r] = total;
        info[r] = n_out | (n_solid << 12) | (s0 << 31);   // at most 1024 segments a ray
    }
}

__global__ __launch_bounds__(256) void k_span_tally(uint32_t n, const uint32_t* __restrict__ counts,
                                                     const uint32_t* __restrict__ info, SpanState* __restrict__ st) {
    // whole waves run to the end (the sums cover the wave)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t c_out = 0, c_solid = 0, c_spans = 0, c_rays = 0, c_in = 0;
    if (i < n) {
        const uint32_t w = info[i];
        c_out = w & 0xfffu;
        c_solid = (w >> 12) & 0xfffu;
        c_in = w >> 31;
        c_spans = counts[i];
        c_rays = c_spans ? 1u : 0u;
    }
    c_out = wave_sum(c_out);
    c_solid = wave_sum(c_solid);
    c_rays = wave_sum(c_rays);
    c_in = wave_sum(c_in);
    // a wave's spans: at most 64 (32 nseg + 1) < 2^22
    c_spans = wave_sum(c_spans);
    if ((threadIdx.x & 63u) == 0u) {
        if (c_out) atomicAdd(&st->outside, (u64)c_out);
        if (c_solid) atomicAdd(&st->solid, (u64)c_solid);
        if (c_spans) atomicAdd(&st->spans, (u64)c_spans);
        if (c_rays) atomicAdd(&st->rays, (u64)c_rays);
        if (c_in) atomicAdd(&st->inside, (u64)c_in);
    }
}

// exclusive wave prefix of v; total = the wave's sum, as a scalar
__device__ __forceinline__ uint32_t wave_excl(uint32_t v, int lane, uint32_t& total) {
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
        if (lane >= o) x += y;
    }
    total = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)x, 63, 64));
    return x - v;
}

__global__ __launch_bounds__(256) void k_span_emit(uint32_t n, int N, const uint64_t* __restrict__ words,
                                                    const uint32_t* __restrict__ info, const uint32_t* __restrict__ offsets,
                                                    int32_t* __restrict__ kk, uint32_t* __restrict__ ray_of) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t r = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= n) return;
    const uint32_t base = offsets[r], total = offsets[r + 1] - base;   // the ray's spans: kk[2 base .. 2 (base + total))
    if (total == 0) return;
    const int nseg = (N + kSeg - 1) / kSeg;
    const uint64_t* __restrict__ w_r = words + (size_t)r * (size_t)nseg;
    const uint32_t s0 = info[r] >> 31;
    uint32_t n_in = s0, n_exit = 0;   // entries and exits written so far (wave-uniform)
    if (s0 && lane == 0) {
        kk[2 * (size_t)base] = 0;
        ray_of[base] = r;
    }
    for (int j0 = 0; j0 < nseg; j0 += 64) {
        const int seg = j0 + lane;
        const bool valid = seg < nseg;
        const uint64_t w = valid ? w_r[seg] : 0ull;
        const uint64_t prev = !valid ? 0ull : seg == 0 ? (uint64_t)s0 : w_r[seg - 1] >> 63;
        const uint64_t x = w ^ ((w << 1) | prev);
        uint64_t rise = x & w, fall = x & ~w;   // behind a partial segment's last sample: an exit at N + 1
        uint32_t t_in, t_exit;
        uint32_t p_in = n_in + wave_excl((uint32_t)__popcll((u64)rise), lane, t_in);
        uint32_t p_exit = n_exit + wave_excl((uint32_t)__popcll((u64)fall), lane, t_exit);
        // the ranks stay below total when the words are the ones the counts were taken from; checked all the same
        while (rise) {
            const int i = __builtin_ctzll((u64)rise);
            rise &= rise - 1ull;
            if (p_in < total) {
                kk[2 * (size_t)(base + p_in)] = kSeg * seg + 1 + i;
                ray_of[base + p_in] = r;
            }
            ++p_in;
        }
        while (fall) {
            const int i = __builtin_ctzll((u64)fall);
            fall &= fall - 1ull;
            if (p_exit < total) kk[2 * (size_t)(base + p_exit) + 1] = kSeg * seg + 1 + i;
            ++p_exit;
        }
        n_in += t_in;
        n_exit += t_exit;
    }
    // a full last segment that ends solid: the ray ends inside
    if (n_exit < total && lane == 0) kk[2 * (size_t)(base + total - 1u) + 1] = N + 1;
}

template <int D>
__global__ __launch_bounds__(256) void k_span_refine(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                      float2 tab_range, const float* __restrict__ ts,
                                                      const float* __restrict__ org, const float* __restrict__ dir, int N, int B,
                                                      int prune, uint32_t n_ends, const int32_t* __restrict__ kk,
                                                      const uint32_t* __restrict__ ray_of, float* __restrict__ t_out,
                                                      float* __restrict__ f_out, float* __restrict__ normals) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;   // end e: span e / 2, its entry (even) or exit (odd)
    if (e >= n_ends) return;
    const bool is_exit = (e & 1u) != 0u;
    // an entry: 0 .. N; an exit: 1 .. N + 1 (emit writes nothing else; the clamp keeps every index below in its table)
    const int k = is_exit ? min(max(kk[e], 1), N + 1) : min(max(kk[e], 0), N);
    const RayAt ray = ray_at(org, dir, ray_of[e >> 1]);
    const int nseg = (N + kSeg - 1) / kSeg;
    const bool bracket = is_exit ? k <= N : k >= 1;
    // the solid end and the other end of the bracket [ts[k - 1], ts[k]]; without one: ts[0] or ts[N]
    const int ks = is_exit ? k - 1 : k, ko = is_exit ? min(k, N) : max(k - 1, 0);
    uint64_t m = 0;
    if (prune) {
        bool fin;
        (void)bound_segment<D>(prog, tab, tab_range, ts, ray, min(max(k - 1, 0) / kSeg, nseg - 1), N, m, fin);
    }
    float t = ts[ks], o = ts[ko], f = 0.f;
    const int rounds = bracket ? B : 0;
    float x = t;
    for (int round = -1; round < rounds; ++round) {
        if (round >= 0) {
            // m = a + 0.5f * (b - a) with a the lower end: an entry's other end, an exit's solid end
            const float a = is_exit ? t : o, b = is_exit ? o : t;
            x = a + 0.5f * (b - a);
            if (x == a || x == b) break;   // every later round repeats this one
        }
        const V3 p = ray_point(ray, x);
        const float fx = ray_field<D>(prog, tab, m, p);
        if (round < 0 || !(fx < 0.f)) {
            t = x;
            f = fx;
        } else {
            o = x;
        }
    }
    t_out[e] = t;
    f_out[e] = f;
    if (normals) {
        V3 nrm{0.f, 0.f, 0.f};
        const V3 p = ray_point(ray, t);
        (void)ob::vertex_normal_at(ob::InterpPt<D>{prog, tab}, p.x, p.y, p.z, nrm);
        normals[3 * (size_t)e] = nrm.x;
        normals[3 * (size_t)e + 1] = nrm.y;
        normals[3 * (size_t)e + 2] = nrm.z;
    }
}

void check_chunk(uint32_t n, int N, int B) {
    if (n < 1u || n > kRayMaxChunk) throw std::runtime_error("ray_spans: chunk size out of range");
    if (N < 1 || N > kRayMaxSteps || B < 0 || B > kRayMaxBisect) throw std::runtime_error("ray_spans: steps or bisect out of range");
    if ((uint64_t)n * (uint64_t)((N + kSeg - 1) / kSeg) > kSpanMaxWords) throw std::runtime_error("ray_spans: chunk beyond the scratch budget");
}

}  // namespace

void launch_span_march(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_ts,
                       const float* d_org, const float* d_dir, uint32_t n, int N, bool prune, uint64_t* d_words,
                       uint32_t* d_counts, uint32_t* d_info, hipStream_t s) {
    check_chunk(n, N, 0);
    const unsigned blocks = (n + 3u) / 4u;
    const int D = eval_depth(prog_depth), p = prune ? 1 : 0;
#define IMPLI_SPAN_MARCH(DD) \
    k_span_march<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, tab_range, d_ts, d_org, d_dir, n, N, p, d_words, d_counts, d_info)
    if (D <= 4) IMPLI_SPAN_MARCH(4);
    else if (D <= 8) IMPLI_SPAN_MARCH(8);
    else if (D <= 12) IMPLI_SPAN_MARCH(12);
    else IMPLI_SPAN_MARCH(16);
#undef IMPLI_SPAN_MARCH
}

void launch_span_tally(uint32_t n, const uint32_t* d_counts, const uint32_t* d_info, SpanState* d_state, hipStream_t s) {
    if (n < 1u || n > kRayMaxChunk) throw std::runtime_error("ray_spans: chunk size out of range");
    k_span_tally<<<(n + 255u) / 256u, 256, 0, s>>>(n, d_counts, d_info, d_state);
}

void launch_span_emit(uint32_t n, int N, const uint64_t* d_words, const uint32_t* d_info, const uint32_t* d_offsets,
                      int32_t* d_k, uint32_t* d_ray_of, hipStream_t s) {
    check_chunk(n, N, 0);
    k_span_emit<<<(n + 3u) / 4u, 256, 0, s>>>(n, N, d_words, d_info, d_offsets, d_k, d_ray_of);
}

void launch_span_refine(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_ts,
                        const float* d_org, const float* d_dir, int N, int B, bool prune, uint32_t n_spans, const int32_t* d_k,
                        const uint32_t* d_ray_of, float* d_t, float* d_f, float* d_normals, hipStream_t s) {
    check_chunk(1u, N, B);
    if (n_spans < 1u || n_spans >= (1u << 30)) throw std::runtime_error("ray_spans: span count out of range");
    const uint32_t n_ends = 2u * n_spans;
    const unsigned blocks = (n_ends + 255u) / 256u;
    const int D = eval_depth(prog_depth), p = prune ? 1 : 0;
#define IMPLI_SPAN_REFINE(DD) \
    k_span_refine<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, tab_range, d_ts, d_org, d_dir, N, B, p, n_ends, d_k, d_ray_of, d_t, d_f, d_normals)
    if (D <= 4) IMPLI_SPAN_REFINE(4);
    else if (D <= 8) IMPLI_SPAN_REFINE(8);
    else if (D <= 12) IMPLI_SPAN_REFINE(12);
    else IMPLI_SPAN_REFINE(16);
#undef IMPLI_SPAN_REFINE
}

}  // namespace impli
