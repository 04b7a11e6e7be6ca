// eval_bricks.hpp -- device side of the brick-pruned field evaluation, shared by the static
// interpreter kernels (eval.hip) and the JIT-compiled tree kernels (jit.cpp).
#pragma once
#include "grid.hpp"

// evaluate a brick's two layers as one straight-line block (measured 57 -> 45 us at 512^3 on the
// config-4 tree); IMPLISOLID_EVAL_PAIR=0 in the environment compiles the JIT kernels without it.
// eval_bricks_body's Pair parameter chooses per kernel (the merged interpreter launch: off)
#ifndef IMPLI_EVAL_PAIR
#define IMPLI_EVAL_PAIR 1
#endif

namespace impli {

// one brick row of sign bits
template <int W> struct SignPiece;
template <> struct SignPiece<8> { typedef uint8_t type; };
template <> struct SignPiece<16> { typedef uint16_t type; };
template <> struct SignPiece<32> { typedef uint32_t type; };
typedef SignPiece<kBX>::type sign_piece_t;

// sample coordinate of stored index i (sample i + 1) along an axis (prepare_grid,
// marching_cubes.hpp:1691-1693: x * factor + min - 2 * width)
__device__ __forceinline__ float sample_xy(const GridDesc& g, int axis, int i) {
    return ((float)(i + 1) * g.w[axis] + g.lo[axis]) - 2.f * g.w[axis];
}
__device__ __forceinline__ float sample_z(const GridDesc& g, int layer) {
    return ((float)(g.fz0 + layer) * g.w[2] + g.lo[2]) - 2.f * g.w[2];
}
// seal_exterior (:895-963): samples 1 and res-2 of any axis hold -1e7
__device__ __forceinline__ bool sealed_xy(const GridDesc& g, int i) { return i == 0 || i == g.n - 1; }
__device__ __forceinline__ bool sealed_z(const GridDesc& g, int layer) {
    const int sz = g.fz0 + layer;
    return sz == 1 || sz == g.res - 2;
}
constexpr float kSealed = -10000000.0f;

__device__ __forceinline__ void brick_of(int b, const BrickGrid& bg, int& bx, int& by, int& bz) {
    bx = b % bg.nbx;
    const int t = b / bg.nbx;
    by = t % bg.nby;
    bz = t / bg.nby;
}

// One wave per listed brick (kBX x kBY lanes, kBZ layers each; grid-stride over the list built by
// k_brick_fill, modes[i] the listed brick's pruning modes): every sample is evaluated with
// `ev(modes, x, y, z)`, stored, and its sign bit set (wave ballot: 64 bits = kBY rows x kBX
// samples).  Sign-filled bricks never reach this kernel -- k_brick_fill wrote their constant sign
// bits -- except claimed candidates (grid.hpp ClaimCtx), evaluated by the wave of the mixed brick
// that claimed them, values only (their sign pieces are constant and already written).
// both layers of a column: the evaluator's pair() when it has one (the JIT tree: one pass of the
// tree code for both samples), else two calls
template <class Eval>
__device__ __forceinline__ auto eval_pair(const Eval& ev, uint64_t m, float x, float y, float z0, float z1, float& f0,
                                          float& f1, int) -> decltype(ev.pair(m, x, y, z0, z1, f0, f1), void()) {
    ev.pair(m, x, y, z0, z1, f0, f1);
}
template <class Eval>
__device__ __forceinline__ void eval_pair(const Eval& ev, uint64_t m, float x, float y, float z0, float z1, float& f0,
                                          float& f1, long) {
    f0 = ev(m, x, y, z0);
    f1 = ev(m, x, y, z1);
}

// The JIT kernel's arguments are one EvalBricksArgs (grid.hpp) by value: its kernarg segment.  Kept
// in SGPRs across the tree code they were parked in VGPR lanes (a lane write or read plus a hazard
// slot each): the JIT evaluator reads them again where they are used, with scalar loads from the
// kernarg segment that cost no vector slot (kernarg_again; JitEval::again in jit.cpp takes the
// offsets from the struct that is the kernel's parameter, so they cannot drift from it).
// T at byte offset `off` of the calling kernel's kernarg segment, loaded anew: the empty asm (no
// instruction) hides the pointer's origin, so the loads are not merged with earlier ones
template <class T>
__device__ __forceinline__ T kernarg_again(unsigned off) {
    const __attribute__((address_space(4))) char* p =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    static_assert(sizeof(T) % 4 == 0, "whole words");
    // word by word through the constant address space (scalar loads; the unused ones go away)
    const __attribute__((address_space(4))) uint32_t* src = (const __attribute__((address_space(4))) uint32_t*)(p + off);
    uint32_t w[sizeof(T) / 4];
#pragma unroll
    for (unsigned k = 0; k < sizeof(T) / 4; ++k) w[k] = src[k];
    T v;
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}
// a pointer read that way is a kernel argument like the first copy: global memory, not generic
// (through its integer value: a global address is the same number in both address spaces, and a
// plain cast there and back folds away)
template <class T>
__device__ __forceinline__ T* as_global(T* p) { return (T*)(__attribute__((address_space(1))) T*)(uint64_t)p; }
// whether the evaluator re-reads the kernel's arguments (ev.again(v): the JIT kernel's evaluator;
// the interpreter kernels' evaluators do not, and run eval_listed as it always was)
template <class Eval, class = void> struct HasAgain { static constexpr bool value = false; };
template <class Eval>
struct HasAgain<Eval, decltype(static_cast<const Eval*>(nullptr)->again(*static_cast<const GridDesc*>(nullptr)), void())> {
    static constexpr bool value = true;
};

// one brick (b, its modes m) by the calling wave; neg[k]: layer k's sign bits, valid: the lanes
// inside the grid
template <class Eval, bool Pair = IMPLI_EVAL_PAIR != 0>
__device__ __forceinline__ void eval_one_brick(const Eval& ev, const GridDesc& g, const BrickGrid& bg, int b, uint64_t m64,
                                               float* __restrict__ field, sign_piece_t* __restrict__ signs,
                                               bool write_signs, uint64_t neg[kBZ], uint64_t& valid) {
    const int lane = threadIdx.x & 63;
    const int n = g.n;
    const int layers = g.fz1 - g.fz0;
    const int row_pieces = (64 / kBX) * sign_row_words(g);
    int bx, by, bz;
    brick_of(b, bg, bx, by, bz);
    const int sx = bx * kBX + (lane % kBX), sy = by * kBY + (lane / kBX);
    const bool ok = sx < n && sy < n;
    valid = __ballot(ok);
    const bool sealed_col = sealed_xy(g, sx) || sealed_xy(g, sy);
    // brick-major field (grid.hpp field_index): the brick's layer k is 64 consecutive floats, one
    // per lane -- the wave stores two whole lines (lanes past the grid edge fill the padding)
    float* out = field + (size_t)b * kBrickSamples + lane;
    const uint64_t m = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(m64 >> 32)) << 32) |
                       (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)m64);
    const float x = sample_xy(g, 0, ok ? sx : 0), y = sample_xy(g, 1, ok ? sy : 0);
#pragma unroll
    for (int k = 0; k < kBZ; ++k) neg[k] = 0;
    if constexpr (Pair) {
        // both layers' tree evaluations in one straight-line block: two independent dependency
        // chains per lane (a layer past the slab is evaluated at a clamped z and not stored)
        static_assert(!Pair || kBZ == 2, "the layer pair needs two layers per brick");
        const int l0 = bz * kBZ, l1 = l0 + 1;
        float f0, f1;
        eval_pair(ev, m, x, y, sample_z(g, l0), sample_z(g, l1 < layers ? l1 : l0), f0, f1, 0);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int layer = l0 + k;
            if (layer >= layers) break;
            const float v = (sealed_col || sealed_z(g, layer)) ? kSealed : 0.f + (k ? f1 : f0);
            out[k * kBX * kBY] = v;
            neg[k] = __ballot(v < 0.f);
            if (write_signs && lane < kBY) {
                const int yy = by * kBY + lane;
                if (yy < n) signs[((size_t)layer * n + yy) * row_pieces + bx] = (sign_piece_t)(neg[k] >> (kBX * lane));
            }
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < kBZ; ++k) {
            const int layer = bz * kBZ + k;
            if (layer >= layers) break;
            const float f = ev(m, x, y, sample_z(g, layer));
            const float v = (sealed_col || sealed_z(g, layer)) ? kSealed : 0.f + f;
            out[k * kBX * kBY] = v;
            const uint64_t nk = __ballot(v < 0.f);
            neg[k] = nk;
            if (write_signs && lane < kBY) {
                const int yy = by * kBY + lane;
                if (yy < n) signs[((size_t)layer * n + yy) * row_pieces + bx] = (sign_piece_t)(nk >> (kBX * lane));
            }
        }
    }
}

// The face neighbours of a just evaluated mixed brick that it claims (bit d: direction d = -x, +x,
// -y, +y, -z, +z): candidates (grid.hpp) of sign s such that some sample of this brick on the
// shared face has the other sign -- a cell edge across the face changes sign there, so marching
// cubes reads the candidate's value -- and that no other wave claimed first (atomic on the fill
// byte).  Face samples are the lanes of the face column / row in both layers, or a whole layer.
//
// One direction per lane: lane d < 6 owns direction d, so everything per direction is one vector
// instruction over those lanes -- one load of the six fill bytes, one atomic for all the claims --
// and the wave's chain after its tree code is two memory round trips: the fill bytes, then the
// atomics together with the candidates' modes (Modes: ccls, bmodes and cmodes loaded through clamped
// indices in the same issue group as the atomic; m_lane: lane d's candidate's modes, read by the
// caller with lane_modes).  The other lanes run direction 0's arithmetic on the brick itself.
struct ClaimLane {
    int ax;         // the lane's axis and side (direction d = 2 ax + up; lanes past 5: direction 0)
    bool up;
    int an;         // the lane's neighbour brick, the brick itself where that is outside the grid
    int cx, cy, cz; // its brick coordinates
};
// The lane's index where a claim is made, opaque to the optimiser (an empty asm: no instruction).
// What the claim derives from it alone -- the lane's direction, its axis tests, its face masks -- is
// invariant in the brick loop; hoisted out of it, it was kept across the tree code (nine VGPRs, six
// SGPR pairs, two of them spilled: 18 -> 22 spilled SGPRs in the baked config-4 module).
__device__ __forceinline__ int claim_lane_index() {
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    return lane;
}
__device__ __forceinline__ ClaimLane claim_lane(const BrickGrid& bg, int b, int lane) {
    int bx, by, bz;
    brick_of(b, bg, bx, by, bz);
    const int d = lane < 6 ? lane : 0;
    const int ax = d >> 1;
    const bool up = d & 1;
    const int c = ax == 0 ? bx : ax == 1 ? by : bz;
    const int lim = ax == 0 ? bg.nbx : ax == 1 ? bg.nby : bg.nbz;
    const int step = ax == 0 ? 1 : ax == 1 ? bg.nbx : bg.nbx * bg.nby;
    const int room = up ? lim - 1 - c : c;   // bricks between this one and the grid's face (selects, no branch)
    const bool in = (lane < 6) & (room > 0);
    const int dl = in ? (up ? 1 : -1) : 0;
    return ClaimLane{ax, up, b + dl * step, bx + (ax == 0 ? dl : 0), by + (ax == 1 ? dl : 0), bz + (ax == 2 ? dl : 0)};
}
// direction d's modes out of the per-lane pair (d wave-uniform)
__device__ __forceinline__ uint64_t lane_modes(uint64_t m_lane, int d) {
    return ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(m_lane >> 32), d) << 32) |
           (uint64_t)__builtin_amdgcn_readlane((uint32_t)m_lane, d);
}
template <bool Modes>
__device__ __forceinline__ uint32_t claim_neighbours(const GridDesc& g, const BrickGrid& bg, const ClaimCtx& cc, int b,
                                                     const uint64_t neg[kBZ], uint64_t valid, uint64_t& m_lane) {
    static_assert(kBZ == 2, "face masks of two-layer bricks");
    const int lane = claim_lane_index();
    const ClaimLane cl = claim_lane(bg, b, lane);
    // round trip 1: the lane's neighbour's fill byte (a neighbour outside the grid reads the brick's
    // own byte, which is never a candidate: it is listed)
    const uint32_t fa = cc.fill[cl.an];
    const int layers = g.fz1 - g.fz0;
    const bool has1 = (b / (bg.nbx * bg.nby)) * kBZ + 1 < layers;
    uint64_t col0 = 0, row0 = (1ull << kBX) - 1ull;
#pragma unroll
    for (int r = 0; r < kBY; ++r) col0 |= 1ull << (r * kBX);
    // the lane's face: its samples in layer 0 and in layer 1
    const int ax = cl.ax;
    const bool up = cl.up;
    const uint64_t fxy = (ax == 0 ? col0 : row0) << (up ? (ax == 0 ? kBX - 1 : kBX * (kBY - 1)) : 0);
    const uint64_t fz = up ? 0ull : ~0ull;
    uint64_t f0 = ax == 2 ? fz : fxy, f1 = ax == 2 ? ~fz : fxy;
    f0 &= valid;
    f1 = has1 ? (f1 & valid) : 0ull;
    // a candidate neighbour with a sample of the other sign on the shared face
    const uint64_t flip = (fa & 3u) == kBrickNeg ? ~0ull : 0ull;
    const uint64_t differ = ((neg[0] ^ flip) & f0) | ((neg[1] ^ flip) & f1);
    const bool want_l = lane < 6 && (fa & kBrickCandidate) && cl.an != b && differ != 0ull;
    const uint32_t want = (uint32_t)__ballot(want_l);
    if (!want) return 0u;   // uniform
    // round trip 2, one issue group: every lane's candidate's modes (unconditional, selected after)
    // and the wanted lanes' claims as one atomic instruction.  Two directions in one 32-bit word are
    // two lanes' atomics on one address: each sets its own byte and reads its own byte's old flag.
    uint32_t cls = 0;
    uint64_t bm = 0, cm = 0;
    if constexpr (Modes) {
        const int cb = cl.cx + cl.cy * cc.cnbx + (cl.cz / kCZ) * cc.cplane;
        cls = cc.ccls[cb];
        bm = cc.bmodes[cl.an];
        cm = cc.cmodes[cb];
    }
    const uint32_t shift = 8u * ((uint32_t)cl.an & 3u);
    uint32_t old = 0u;
    if (want_l) old = atomicOr(reinterpret_cast<uint32_t*>(cc.fill + (cl.an & ~3)), (uint32_t)kBrickClaimed << shift);
    // the branch holds the atomic alone: its result is first read here, past the join (an empty asm,
    // no instruction).  Without it the modes' select was copied into both sides of the branch, each
    // with its own wait, and the atomic was issued only after the other side's loads had come back.
    asm volatile("" : "+v"(old));
    if constexpr (Modes) m_lane = cls == kBrickMixed ? bm : cm;
    return (uint32_t)__ballot(want_l && !((old >> shift) & kBrickClaimed));   // first claimer wins
}

// a listed entry: the brick, then (mixed bricks) the candidates it claimed, with their own modes --
// one loop around a single copy of the tree code
template <class Eval, bool Pair = IMPLI_EVAL_PAIR != 0>
__device__ __forceinline__ void eval_listed(const Eval& ev, const GridDesc& g, const BrickGrid& bg, const ClaimCtx& cc,
                                            uint32_t entry, uint64_t m64, float* __restrict__ field,
                                            sign_piece_t* __restrict__ signs) {
    const int b = (int)(entry & ~kListCheck);
    const bool check = (entry & kListCheck) && cc.fill;
    int cur = b;
    uint64_t mcur = m64, m_lane = 0;
    uint32_t claimed = 0;
    for (bool first = true;; first = false) {
        uint64_t neg[kBZ], valid;
        eval_one_brick<Eval, Pair>(ev, g, bg, cur, mcur, field, signs, first, neg, valid);
        if (first && check) claimed = claim_neighbours<true>(g, bg, cc, b, neg, valid, m_lane);
        if (!claimed) break;
        // the next claimed direction: its brick, and its modes from lane d (no loads in this loop)
        const int d = __builtin_ctz(claimed);
        claimed &= claimed - 1u;
        const int ax = d >> 1, up = d & 1;
        const int step = ax == 0 ? 1 : ax == 1 ? bg.nbx : bg.nbx * bg.nby;
        cur = up ? b + step : b - step;
        mcur = lane_modes(m_lane, d);
    }
}

// eval_one_brick's layer pair for an evaluator that re-reads the kernel's arguments: nothing of
// them is live across the tree code
template <class Eval>
__device__ __forceinline__ void eval_one_brick_again(const Eval& ev, const GridDesc& g, const BrickGrid& bg, int b,
                                                     uint64_t m64, const StorePtrs& ptrs, bool write_signs,
                                                     uint64_t neg[kBZ], uint64_t& valid) {
    static_assert(kBZ == 2, "the layer pair needs two layers per brick");
    const int lane = threadIdx.x & 63;
    int bx, by, bz;
    brick_of(b, bg, bx, by, bz);
    const int sx = bx * kBX + (lane % kBX), sy = by * kBY + (lane / kBX);
    const uint64_t m = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(m64 >> 32)) << 32) |
                       (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)m64);
    const int l0 = bz * kBZ, l1 = l0 + 1;
    float f0, f1;
    {   // before the tree code: the sample coordinates
        const GridDesc ga = ev.again(g);
        const bool ok = sx < ga.n && sy < ga.n;
        const float x = sample_xy(ga, 0, ok ? sx : 0), y = sample_xy(ga, 1, ok ? sy : 0);
        eval_pair(ev, m, x, y, sample_z(ga, l0), sample_z(ga, l1 < ga.fz1 - ga.fz0 ? l1 : l0), f0, f1, 0);
    }
    // after it: what the stores need
    const GridDesc gs = ev.again(g);
    const StorePtrs sp = ev.again(ptrs);
    float* __restrict__ const field = sp.field;
    sign_piece_t* __restrict__ const signs = static_cast<sign_piece_t*>(sp.signs);
    const int n = gs.n, layers = gs.fz1 - gs.fz0, row_pieces = (64 / kBX) * sign_row_words(gs);
    valid = __ballot(sx < n && sy < n);
    const bool sealed_col = sealed_xy(gs, sx) || sealed_xy(gs, sy);
    float* out = field + (size_t)b * kBrickSamples + lane;
    neg[0] = neg[1] = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int layer = l0 + k;
        if (layer >= layers) break;
        const float v = (sealed_col || sealed_z(gs, layer)) ? kSealed : 0.f + (k ? f1 : f0);
        out[k * kBX * kBY] = v;
        neg[k] = __ballot(v < 0.f);
        if (write_signs && lane < kBY) {
            const int yy = by * kBY + lane;
            if (yy < n) signs[((size_t)layer * n + yy) * row_pieces + bx] = (sign_piece_t)(neg[k] >> (kBX * lane));
        }
    }
}

// eval_listed for such an evaluator.  The claim takes the loop-carried cur (equal to b in the first
// iteration, the only one that claims): given b, its brick arithmetic -- six neighbour addresses,
// in-grid flags, atomic words and shifts -- is invariant in this loop, was hoisted above the tree
// code and lived across it in 45 VGPR lanes.  cur is wave-uniform and said so, or instruction
// selection moves its whole chain (brick_of's divisions, the addresses) to the vector unit.
template <class Eval>
__device__ __forceinline__ void eval_listed_again(const Eval& ev, const GridDesc& g, const BrickGrid& bg, const ClaimCtx& cc,
                                                  uint32_t entry, uint64_t m64, const StorePtrs& ptrs) {
    const int b = (int)(entry & ~kListCheck);
    const bool check = (entry & kListCheck) && cc.fill;
    int cur = b;
    uint64_t mcur = m64, m_lane = 0;
    uint32_t claimed = 0;
    for (bool first = true;; first = false) {
        uint64_t neg[kBZ], valid;
        cur = __builtin_amdgcn_readfirstlane(cur);
        eval_one_brick_again(ev, g, bg, cur, mcur, ptrs, first, neg, valid);
        if (first && check) claimed = claim_neighbours<true>(ev.again(g), bg, ev.again(cc), cur, neg, valid, m_lane);
        if (!claimed) break;
        const int d = __builtin_ctz(claimed);
        claimed &= claimed - 1u;
        const int ax = d >> 1, up = d & 1;
        const int step = ax == 0 ? 1 : ax == 1 ? bg.nbx : bg.nbx * bg.nby;
        cur = up ? b + step : b - step;
        mcur = lane_modes(m_lane, d);
    }
}

// The same entry without evaluating the claimed candidates in this wave: they are appended to
// `claimed` (one atomic per claiming wave) for a second pass (eval.hip k_eval_claimed_b).  The
// merged object-stream eval runs the interpreter, whose candidate loop kept its state live across a
// second tree evaluation: 227 -> 196 VGPRs without it at stack depth 12, and at depth 9 168 -- three
// waves per SIMD instead of two.
template <class Eval, bool Pair = IMPLI_EVAL_PAIR != 0>
__device__ __forceinline__ void eval_listed_deferred(const Eval& ev, const GridDesc& g, const BrickGrid& bg,
                                                     const ClaimCtx& cc, uint32_t entry, uint64_t m64,
                                                     float* __restrict__ field, sign_piece_t* __restrict__ signs,
                                                     uint32_t* __restrict__ claimed_list, uint32_t* __restrict__ claimed_count,
                                                     uint32_t claimed_cap) {
    const int b = (int)(entry & ~kListCheck);
    const bool check = (entry & kListCheck) && cc.fill;
    uint64_t neg[kBZ], valid;
    eval_one_brick<Eval, Pair>(ev, g, bg, b, m64, field, signs, true, neg, valid);
    if (!check) return;
    uint64_t unused;   // the second pass loads a candidate's modes itself
    const uint32_t claimed = claim_neighbours<false>(g, bg, cc, b, neg, valid, unused);
    if (!claimed) return;   // uniform
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(claimed_count, (uint32_t)__popc(claimed));
    base = __builtin_amdgcn_readfirstlane(base);
    // lane d < 6 writes direction d's neighbour if claimed, at its rank among the claimed ones
    if (lane < 6 && ((claimed >> lane) & 1u)) {
        int bx, by, bz;
        brick_of(b, bg, bx, by, bz);
        const int ax = lane >> 1, up = lane & 1;
        const int step = ax == 0 ? 1 : ax == 1 ? bg.nbx : bg.nbx * bg.nby;
        const uint32_t at = base + (uint32_t)__popc(claimed & ((1u << lane) - 1u));
        if (at < claimed_cap) claimed_list[at] = (uint32_t)(up ? b + step : b - step);
    }
}

template <class Eval, bool Pair = IMPLI_EVAL_PAIR != 0>
__device__ __forceinline__ void eval_bricks_body(const Eval& ev, const GridDesc& g, const BrickGrid& bg,
                                                 const ClaimCtx& cc, const uint64_t* __restrict__ modes,
                                                 const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                                                 float* __restrict__ field, void* __restrict__ signs_raw) {
    sign_piece_t* signs = static_cast<sign_piece_t*>(signs_raw);
    const uint32_t nb = *count;
    const uint32_t wpb = blockDim.x >> 6;   // waves per block
    const uint32_t stride = gridDim.x * wpb;
    uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * wpb + (threadIdx.x >> 6));
    // the next brick's list entry and modes are loaded while this brick is evaluated
    uint32_t b_next = i < nb ? list[i] : 0u;
    uint64_t m_next = i < nb ? modes[i] : 0ull;
    for (; i < nb; i += stride) {
        const uint32_t e = __builtin_amdgcn_readfirstlane(b_next);
        const uint64_t m64 = m_next;
        if (i + stride < nb) {
            b_next = list[i + stride];
            m_next = modes[i + stride];
        }
        if constexpr (Pair && HasAgain<Eval>::value)
            eval_listed_again(ev, g, bg, cc, e, m64, StorePtrs{field, signs_raw});
        else
            eval_listed<Eval, Pair>(ev, g, bg, cc, e, m64, field, signs);
    }
}

}  // namespace impli
